/* lexls_hip.h — C ABI of the MI355X-native lexicographic-QR core (liblexls_hip.so).
 *
 * The reference (jrl-umi3218/lexls) has no FFI: its boundary for this path is the C++ class
 * LexLS::internal::LexLSE (include/lexls/lexlse.h:33-2886), one object = one problem, all buffers
 * owned by the object.  This ABI is that class turned into a handle over a BATCH of independent
 * problems of the same capacity (the solver's intended workload: successive IK-style instances),
 * each entry point citing the member function it replaces.  Plain pointers and sizes only; no C++
 * or torch types cross the boundary; errors are status codes + lexls_last_error(), never exceptions.
 *
 * Data layout (identical to the reference's storage, lexlse.h:85): one problem is a column-major
 * cap x (nVar+1) array "LOD" with leading dimension cap = sum(maxObjDim); rows [0, nCtr) hold the
 * stacked levels [A_k | b_k] (column nVar = right-hand side).  A batch is `batch` such arrays
 * back to back.  Index = uint32_t, RealScalar = double (typedefs.h:16-17).
 *
 * Host pointers are named h_*, device pointers d_*.  All device work is enqueued on the handle's
 * HIP stream (default: the null stream); calls that return data to the host synchronise that stream.
 */
#ifndef LEXLS_HIP_H
#define LEXLS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lexls_lse_s *lexls_lse_t;

enum lexls_status
{
    LEXLS_OK              = 0,
    LEXLS_ERR_INVALID     = 1, /* bad argument / call order (the reference throws LexLS::Exception) */
    LEXLS_ERR_HIP         = 2, /* a HIP runtime call failed (message has the HIP error string)      */
    LEXLS_ERR_UNSUPPORTED = 3, /* feature of the reference that has no device path yet              */
    LEXLS_ERR_NO_DEVICE   = 4  /* no usable GPU: there is NO CPU fallback in this library           */
};

/* which device array lexls_lse_device_ptr returns */
enum lexls_array
{
    LEXLS_ARRAY_X = 0,      /* double   batch x nVar            solution                              */
    LEXLS_ARRAY_FACTOR,     /* double   batch x cap x (nVar+1)  factor ("lexqr")                      */
    LEXLS_ARRAY_HH,         /* double   batch x cap             Householder scalars                   */
    LEXLS_ARRAY_PERM,       /* uint32   batch x nVar            column_permutations                   */
    LEXLS_ARRAY_RANK,       /* uint32   batch x nObj            obj_info[k].rank                      */
    LEXLS_ARRAY_FIRST_COL,  /* uint32   batch x nObj            obj_info[k].first_col_index           */
    LEXLS_ARRAY_TOTAL_RANK, /* uint32   batch                   TotalRank                             */
    LEXLS_ARRAY_V,          /* double   batch x cap             residuals (get_v)                     */
    LEXLS_ARRAY_LAMBDA,     /* double   batch x (nVar+cap)      [lambda_fixed; lambda] of the last sensitivity call */
    LEXLS_ARRAY_INPUT,      /* double   batch x cap x (nVar+1)  library-owned input buffer            */
    LEXLS_ARRAY_GUARD_ESTIMATE, /* double batch                 accuracy guard: estimate of the last solve (lexls_lse_set_accuracy_guard) */
    LEXLS_ARRAY_GUARD_STATUS,   /* uint8  batch                 accuracy guard: status of the last solve                                  */
    LEXLS_ARRAY_MULTIPLIERS     /* double batch x nObj x (nVar+cap) every objective's multipliers (lexls_lse_multipliers)                 */
};
/* The ids behind LEXLS_ARRAY_MULTIPLIERS continue the numbering of enum lexls_array (the list above is pinned as it stands by
 * tests/test_lsi_lambda_api.py); lexls_lse_device_ptr takes them like the others. */
enum lexls_array_more
{
    LEXLS_ARRAY_WRONG_SIGN = LEXLS_ARRAY_MULTIPLIERS + 1 /* uint8 batch x (nVar+cap) the wrong-sign set of the last lexls_lse_sensitivity_collect call */
};

/* replaces LexLS::Exception::what() (typedefs.h:300-314): no exception crosses the ABI — every entry point returns a status code and
 * leaves the message of the last failure here */
const char *lexls_last_error(void);
int lexls_version(void);

/* number of visible HIP devices; LEXLS_ERR_NO_DEVICE if none */
int lexls_device_count(int *count);

/* ---- lifetime -------------------------------------------------------------------------------- */

/* replaces LexLSE::LexLSE(nVar,nObj,ObjDim) / resize() (lexlse.h:50-103): allocates every device
 * buffer once for `batch` problems of capacity maxObjDim[k] rows per level. */
int lexls_lse_create(lexls_lse_t *out, int device, uint32_t batch, uint32_t nVar, uint32_t nObj, const uint32_t *h_maxObjDim);
int lexls_lse_destroy(lexls_lse_t h);
/* all later work of this handle runs on `hip_stream` (a hipStream_t; NULL = null stream) */
int lexls_lse_set_stream(lexls_lse_t h, void *hip_stream);
int lexls_lse_synchronize(lexls_lse_t h);
/* Deferred synchronisation (lock-step LexLSI batches issue ~10 small copies per active-set round): while on, the set_* / gather / get_*
 * calls only ENQUEUE their copies on the handle's stream.  The caller then owes two things the default mode does not ask for: host input
 * arrays stay untouched, and host output arrays are only read, after the next lexls_lse_synchronize(); and the arrays should be pinned
 * (hipHostMalloc) — with pageable memory the runtime stages the copies and nothing is gained. */
int lexls_lse_set_deferred_sync(lexls_lse_t h, int on);

/* ---- problem definition ----------------------------------------------------------------------- */

/* replaces setParameters (lexlse.h:1467); only REGULARIZATION_NONE has a device path (typedefs.h:122).
 * A CHANGE of the tolerance invalidates what the handle keeps from earlier factorizations: lexls_lse_solve and everything else that needs a
 * kept factor return LEXLS_ERR_INVALID until the next factorization (never the old x), and the prefix-reuse state is dropped — resume levels
 * set before the call are forgotten, lexls_lse_prefix_reuse_ready is 0 and lexls_lse_set_resume_levels an error until a factorization has
 * left a new state (the levels it would read back carry the ranks of the old tolerance).  Setting the same value again changes nothing. */
int lexls_lse_set_tolerance(lexls_lse_t h, double tol_linear_dependence);
/* replaces setObjDim (lexlse.h:1426): h_dims is nObj values (per_problem = 0, same for the whole
 * batch) or batch x nObj values (ragged batch, per_problem = 1); each dims[k] <= maxObjDim[k] */
int lexls_lse_set_obj_dim(lexls_lse_t h, const uint32_t *h_dims, int per_problem);
/* replaces setFixedVariablesCount + fixVariable(s) (lexlse.h:1381-1419, :1449): per problem the
 * number of fixed variables, then (batch x nVar, first nfixed[b] entries used) index / value /
 * ConstraintActivationType.  h_nfixed == NULL clears all fixed variables. */
int lexls_lse_set_fixed(lexls_lse_t h, const uint32_t *h_nfixed, const uint32_t *h_index, const double *h_value, const uint8_t *h_type);
/* activation types of the fixed variables only (batch x nVar bytes, fixVariable order, lexlse.h:1381-1419); unlike lexls_lse_set_fixed
 * it keeps the factorization valid — the types only matter to ObjectiveSensitivity (lexlse.h:866-987 marks CORRECT_SIGN_OF_LAMBDA) */
int lexls_lse_set_fixed_type(lexls_lse_t h, const uint8_t *h_type);
/* replaces setCtrType (lexlse.h:1548): batch x cap ConstraintActivationType bytes, row order of LOD */
int lexls_lse_set_ctr_type(lexls_lse_t h, const uint8_t *h_types);
/* lock-step batches (batched LexLSI): problems whose flag is non-zero are left untouched by the next
 * factorize / factorize_solve calls (their previous results stay valid).  NULL clears the mask; a mask whose bytes are all zero is no
 * mask (the dispatch of an unmasked run, the same bits).  The guarantee covers problems whose dims / fixed variables are those of the
 * skipped run: x, pivots, ranks, the kept factor with its Householder scalars and the accuracy guard's report keep their bits, and the
 * post-factorization calls read the kept factor as the old one.  A skipped problem's input is not read (it may hold anything). */
int lexls_lse_set_skip(lexls_lse_t h, const uint8_t *h_skip);
/* replaces setProblem / setData (lexlse.h:1511-1530): copies batch x cap x (nVar+1) doubles H2D */
int lexls_lse_set_problem_host(lexls_lse_t h, const double *h_lod);
/* zero-copy variant: the caller's device buffer becomes the (read-only) input of later factorizations.  d_lod must be a multiple of
 * 8 bytes (anything else: LEXLS_ERR_INVALID, the handle keeps the input and the factor it had); any such address inside a larger
 * buffer serves, every kernel reads it in the handle's stream.  lqr_qtol's uniform instantiations and lqr_mfma need 16 bytes: on a
 * pointer that is 8 mod 16 they give way to the bit-exact kernel of the shape (lqr_qtol's ragged instantiations, policy 10, do not). */
int lexls_lse_set_problem_device(lexls_lse_t h, const double *d_lod);
/* Device-side assembly of the equality problems of a LexLSI iteration — replaces the row copies of Objective::formLexLSE
 * (objective.h:434-494).  set_constraint_data keeps, per problem, `per_problem` doubles of constraint data
 * resident on the device (the objectives' [A | lb | ub] blocks back to back, each column-major — the flat layout of lexls_lsi_solve);
 * gather_problem then builds every non-skipped problem's LOD from two batch x cap uint32 arrays: row r of the LOD is
 * [ data[src + j*ld], j < nVar | data[src + (nVar + ub)*ld] ] with src = h_row_src[r], ld = h_row_ld[r] & 0x7fffffff,
 * ub = h_row_ld[r] >> 31 (0: right-hand side = lb, 1: ub — objective.h:472-486); rows with h_row_ld[r] == 0 are left alone. */
int lexls_lse_set_constraint_data(lexls_lse_t h, const double *h_data, uint64_t per_problem);
int lexls_lse_gather_problem(lexls_lse_t h, const uint32_t *h_row_src, const uint32_t *h_row_ld);

/* One copy each way per active-set round (lock-step LexLSI batches).  The handle keeps the small per-round arrays in two device slabs;
 * lexls_lse_round_layout gives the byte offset of each array inside them so that a host block of the same layout can be moved with one
 * copy instead of one per array:
 *   in slab  : dims (u32 batch x nObj) | nfixed (u32 batch) | fixed_idx (u32 batch x nVar) | fixed_val (f64 batch x nVar) | skip (u8 batch)
 *              | obj_index (i32 batch) | row_src, row_ld (u32 batch x cap) | fixed_type (u8 batch x nVar) | ctr_type (u8 batch x cap)
 *   out slab : x (f64 batch x nVar) | total_rank (u32 batch) | found (i32 batch x 3) | max_abs (f64 batch)
 * upload_round  = set_obj_dim(per_problem) + set_fixed + set_ctr_type + set_skip + the obj_index of a later sensitivity_resident
 *                 (+ gather_problem when gather != 0), with the same argument checks;
 * download_round: h_out receives the out slab (out_bytes), h_types the tail of the in slab from fixed_type on
 *                 (in_bytes - fixed_type bytes: fixed_type, then ctr_type at offset ctr_type - fixed_type); either may be NULL. */
typedef struct lexls_round_layout
{
    uint64_t in_bytes, dims, nfixed, fixed_idx, fixed_val, skip, obj_index, row_src, row_ld, fixed_type, ctr_type;
    uint64_t out_bytes, x, total_rank, found, max_abs;
} lexls_round_layout;
int lexls_lse_round_layout(lexls_lse_t h, lexls_round_layout *out);
int lexls_lse_upload_round(lexls_lse_t h, const void *h_in, int gather);
int lexls_lse_download_round(lexls_lse_t h, void *h_out, void *h_types);

/* ---- the hot path ------------------------------------------------------------------------------ */

/* replaces factorize() (lexlse.h:117-506): factor, Householder scalars, pivots, ranks on device */
int lexls_lse_factorize(lexls_lse_t h);
/* replaces solve() (lexlse.h:1015-1045); needs a factorization */
int lexls_lse_solve(lexls_lse_t h);
/* factorize()+solve() in one launch per batch; keep_factor = 0 skips writing the factor to HBM
 * (x, ranks and pivots only — the "x-only" traffic variant of SURVEY.md section 8(d)) */
int lexls_lse_factorize_solve(lexls_lse_t h, int keep_factor);
/* replaces solveLeastNorm_1() (lexlse.h:1052-1131, Givens sweep); needs a factorization */
int lexls_lse_solve_least_norm(lexls_lse_t h);
/* replaces setParameters(regularization_type, variable_regularization_factor) + setRegularizationFactor (lexlse.h:1467, :1477;
 * dispatch lexlse.h:277-411).  type: LexLS::RegularizationType — NONE 0, TIKHONOV 1, R 3, R_NO_Z 4, RT_NO_Z 5, TIKHONOV_2 8, TEST 9
 * the CGLS variants TIKHONOV_CG 2, RT_NO_Z_CG 6, and TIKHONOV_1 7 (the type the reference marks experimental: regularize_tikhonov_1_test
 * lexlse.h:1774-1886; its ObjectiveSensitivity then returns the multipliers of the regularized problem, :647-651; generic kernel only;
 * by-products: lexls_lse_get_mu).  h_factors: one factor per level (per_problem == 0) or batch x nObj (per_problem != 0); NULL = all zero. */
int lexls_lse_set_regularization(lexls_lse_t h, int type, const double *h_factors, int per_problem, double variable_factor);
/* max_number_of_CG_iterations (typedefs.h:111, default 10): iteration cap of the two CGLS variants */
int lexls_lse_set_cg_iterations(lexls_lse_t h, uint32_t max_iterations);
/* replaces solveLeastNorm_3() (lexlse.h:1222-1277): least-norm solution from the null-space basis accumulated by the Tikhonov family
 * (regularization type 1, 2, 3 or 8, normally with all factors zero) */
int lexls_lse_solve_least_norm_3(lexls_lse_t h);
/* replaces solveLeastNorm_2() (lexlse.h:1138-1213, normal equations of the free variables + Cholesky); needs a factorization */
int lexls_lse_solve_least_norm_2(lexls_lse_t h);
/* replaces get_v() (lexlse.h:1560-1582); needs a factorization */
int lexls_lse_residual(lexls_lse_t h);
/* replaces bool ObjectiveSensitivity(ObjIndex, CtrIndex2Remove, ObjIndex2Remove, tolWrong, tolCorrect,
 * maxAbsValue) (lexlse.h:611-762) incl. findDescentDirection (:935-987) and its mutation of ctr_type.
 * h_obj_index: one level per problem (batch values; a negative value skips that problem), or NULL
 * with `obj_index_all` applied to every problem.  Results: lexls_lse_get_sensitivity. */
int lexls_lse_sensitivity(lexls_lse_t h, const int32_t *h_obj_index, int32_t obj_index_all, double tol_wrong_sign_lambda, double tol_correct_sign_lambda);
/* While on, lexls_lse_sensitivity(_resident) does what LexLSI's removal search does with one call per level (lexlsi.h:1121-1132): starting
 * at the given level it goes on to the next ones until a level reports a wrong-sign multiplier or the last level is done — one launch; the
 * outputs are those of the level it stopped at.  Off by default (= the reference's one-level call). */
int lexls_lse_set_sensitivity_scan(lexls_lse_t h, int on);
/* same, with the per-problem objective indices already on the device (the obj_index array of lexls_lse_upload_round) */
int lexls_lse_sensitivity_resident(lexls_lse_t h, double tol_wrong_sign_lambda, double tol_correct_sign_lambda);
/* replaces void ObjectiveSensitivity(ObjIndex, tolWrong, tolCorrect, ctr_wrong_sign) (lexlse.h:511-602 around the scan of :866-910), the
 * overload LexLSI's deactivate_first_wrong_sign rule calls (lexlsi.h:1063-1105): the same multipliers (LEXLS_ARRAY_LAMBDA) and the same
 * CORRECT_SIGN_OF_LAMBDA marks in the constraint and fixed-variable types, but instead of the most negative wrong-sign multiplier EVERY one is
 * reported: LEXLS_ARRAY_WRONG_SIGN / lexls_lse_get_wrong_sign, batch x (nVar + cap) bytes per call — bytes [0, nVar) the fixed variables in
 * fixVariable order, bytes [nVar, nVar + cap) the constraint rows in LOD order; 1 where the reference pushes a ConstraintInfo, 0 elsewhere.
 * Scan order: the objective's own level, the levels above it downwards, the fixed variables.  The reference's quirk for the fixed variables is
 * kept (lexlse.h:599-600): min(dims[0], nfixed) entries are scanned, entry k reads the CONSTRAINT multiplier Lambda[k] against fixed type k, and
 * sets byte k.  CONSEQUENCE, known and kept for fidelity to the reference: the true multipliers of the fixed variables are never examined by
 * this rule, so a LexLSI run with deactivate_first_wrong_sign on a hierarchy with simple bounds can end with PROBLEM_SOLVED at a point that is
 * not lexicographically optimal — a simple bound keeps a multiplier of the wrong sign (smallest case found: n = 3, dims (2, 2, 3),
 * tests/test_lexopt_certificate.py; the default rule, lexls_lse_sensitivity, is not affected).  Arguments as lexls_lse_sensitivity; with lexls_lse_set_sensitivity_scan on it goes on to the next objective until one reports a
 * non-empty set or the last is done (the loop of lexlsi.h:1072-1083; marks of the objectives passed stay in place).
 * lexls_lse_get_sensitivity then gives {set non-empty, number of entries, objective the search stopped at} and max_abs = 0 (the reference sets
 * lambda_wrong_sign = 0 on this path); {0, -1, -2} for a problem whose objective index is negative.  _resident: objective indices from the
 * round slab, as lexls_lse_sensitivity_resident. */
int lexls_lse_sensitivity_collect(lexls_lse_t h, const int32_t *h_obj_index, int32_t obj_index_all, double tol_wrong_sign_lambda, double tol_correct_sign_lambda);
int lexls_lse_sensitivity_collect_resident(lexls_lse_t h, double tol_wrong_sign_lambda, double tol_correct_sign_lambda);

/* Every objective's multipliers at once: column k of problem b is what lexls_lse_get_lambda returns after ObjectiveSensitivity(k) — the
 * [lambda_fixed; lambda] workspace head(nMeaningful), nMeaningful = nfixed + dims[0] + ... + dims[k], zero from row nMeaningful on (lexlse.h:611-762,
 * :636-639; the matrix LexLSI::getLambda assembles, lexlsi.h:573-590).  Bit-identical to nObj calls of lexls_lse_sensitivity(k); takes no decisions
 * and leaves the types, the sensitivity outputs and LEXLS_ARRAY_LAMBDA as they are.  Needs a factorization whose factor was kept.  One launch where
 * the removal sweep serves the shape (levels of up to 16 rows, at most 8 objectives, nVar <= 64), else nObj launches.
 * lexls_lse_get_multipliers returns the matrices of the last lexls_lse_multipliers call as long as they belong to the current factor: after a later
 * factorization, or any call that invalidates the factor (a new problem, dimensions, fixed variables, regularization), it fails with
 * LEXLS_ERR_INVALID until lexls_lse_multipliers runs again (LEXLS_ARRAY_MULTIPLIERS keeps the last contents).
 * Layout of h_L (lexls_lse_get_multipliers, LEXLS_ARRAY_MULTIPLIERS): batch x nObj x (nVar + cap) doubles — problem-major, then objective k,
 * then the nVar + cap rows of its column (rows [0, nfixed) the fixed variables in fixVariable order, then the constraint rows of the levels). */
int lexls_lse_multipliers(lexls_lse_t h);
int lexls_lse_get_multipliers(lexls_lse_t h, double *h_L);

/* Adjoint of the solve with respect to the right-hand sides and the fixed values, the matrix A HELD FIXED.  factorize() chooses its pivots and
 * tests the ranks on the columns of A alone (the column norms never see the right-hand-side column), so for fixed A the basic solution is
 * exactly affine in the right-hand sides b and in the values of the fixed variables: x = M b + N x_fixed.  Given g = dloss/dx these calls
 * return grad_rhs = M^T g and grad_fixed = N^T g from one pass over the kept factor (R_k, T_k, the reflectors and their scalars, the Gauss
 * multipliers left in the pivot columns of the lower rows, the permutation, ranks and first columns, the untouched columns of the fixed
 * variables): the reverse of factorize()'s right-hand-side updates and of solve().  There are NO derivatives with respect to A: x is not
 * continuous in A where a rank changes.  Tolerance contract (no reference arithmetic exists); the same bits from run to run.
 * Layouts: g is batch x nVar in the user's variable order (that of lexls_lse_get_x); grad_rhs is batch x cap in LOD row order, zero in the
 * rows behind a problem's own; grad_fixed is batch x nVar, entry j < nfixed the fixed variable of slot j in fixVariable order, zero from
 * nfixed on.
 * lexls_lse_solve_adjoint copies h_g in, launches and keeps the results in buffers of the handle (allocated at the first call);
 * lexls_lse_get_adjoint synchronises and copies them out, either output may be NULL; both follow lexls_lse_set_deferred_sync like the other
 * set / get calls.  lexls_lse_get_adjoint answers only while the results belong to the current factor: after a later factorization, or any
 * call that invalidates the factor, it fails with LEXLS_ERR_INVALID until lexls_lse_solve_adjoint runs again.
 * lexls_lse_solve_adjoint_device reads d_g and writes d_grad_rhs and d_grad_fixed (NULL: not wanted) in device memory: it only enqueues in
 * the handle's stream and makes no host-synchronising call; d_g has to be complete in stream order.
 * Errors, each returned before any device work and with every output left alone: LEXLS_ERR_INVALID for a null handle or a null g (or a
 * null d_grad_rhs); LEXLS_ERR_INVALID when there is no kept factor (an x-only solve, keep_factor = 0, or a tolerance-contract kernel leaves
 * none); LEXLS_ERR_UNSUPPORTED when the factorization ran with regularization_type != 0 and the damped solve is not an affine map of the
 * right-hand side: the CG types 2 and 6 (CGLS from x = 0 with a fixed iteration count), the experimental type 7, and any type with
 * variable_regularization_factor != 0 (the factor then depends on the right-hand side); the message names the condition.
 * After lexls_lse_set_adjoint_regularized(h, 1) — off by default, so that a caller who takes LEXLS_ERR_UNSUPPORTED after a regularized
 * factorization as the sign to differentiate some other way keeps getting it — regularized factorizations of type 1 (TIKHONOV), 3 (R),
 * 4 (R_NO_Z), 5 (RT_NO_Z), 8 (TIKHONOV_2) and 9 (TEST) with variable_regularization_factor == 0 ARE served: their damping is a routine of the level's R and T, the accumulated null-space basis and the
 * factor alone, so with A and the regularization factors held fixed x = M_reg b + N_reg x_fixed is still exactly affine, and the calls return
 * M_reg^T g and N_reg^T g.  The factors are held fixed as A is (those the factorization ran with, shared or per problem, are read from the
 * handle); no gradient with respect to the factors is returned.  They are read from the handle's device array AT THE TIME OF THE ADJOINT CALL:
 * lexls_lse_set_regularization drops the kept factor, so the public setters cannot change them under a factor, but a caller who writes into that
 * array in place (through lexls_lse_device_ptr, or the per-instance device rows of a LexLSI batch) between the factorization and the adjoint gets the adjoint of the
 * rewritten factors, and no error is raised.  Where the hbm variant serves the shape, the first lexls_lse_solve_adjoint(_device) call on the
 * handle allocates its work buffer (a hipMalloc: that one call of the device form is not enqueue-only).
 * Kernel variant (lexls_lse_last_consumer_kernel): "solve_adjoint<64>" without regularization; "solve_adjoint_reg<64,lds>" or
 * "solve_adjoint_reg<64,hbm>" for a served regularized factor — the rebuilt basis, the level's normal equations and the per-level snapshots of
 * the basis in LDS, or in a work buffer of the handle where they exceed one workgroup's 160 KiB (decided from nVar, cap and nObj alone). */
int lexls_lse_solve_adjoint(lexls_lse_t h, const double *h_g);
int lexls_lse_get_adjoint(lexls_lse_t h, double *h_grad_rhs, double *h_grad_fixed);
int lexls_lse_solve_adjoint_device(lexls_lse_t h, const double *d_g, double *d_grad_rhs, double *d_grad_fixed);
/* on != 0: the three calls above serve damped factorizations as their comment says; 0 (the default): LEXLS_ERR_UNSUPPORTED after every
 * regularized factorization.  Takes effect at the next call; the kept factor stays valid.  LEXLS_ERR_INVALID for a null handle. */
int lexls_lse_set_adjoint_regularized(lexls_lse_t h, int on);

/* The same adjoint for MANY cotangents per problem in one pass over the kept factor: ncot vector-Jacobian products, the Jacobian dx/db with the
 * identity as cotangents (ncot = nVar), batched gradients.  One wavefront serves a problem and a tile of up to 64 cotangents, lane = cotangent.
 * Layouts: G is batch x ncot x nVar, cotangent c of problem b in the variable order of lexls_lse_get_x; grad_rhs is batch x ncot x cap in LOD
 * row order, zero in the rows behind a problem's own; grad_fixed is batch x ncot x nVar, zero from nfixed on (NULL: not wanted).
 * lexls_lse_solve_adjoint_multi copies h_G in, launches and keeps the results in buffers of the handle; lexls_lse_get_adjoint_multi copies them
 * out (batch x ncot x cap and batch x ncot x nVar for the ncot of that call, either output may be NULL); both follow
 * lexls_lse_set_deferred_sync, and lexls_lse_get_adjoint_multi answers only while the results belong to the current factor, as
 * lexls_lse_get_adjoint does.  lexls_lse_solve_adjoint_multi_device reads d_G and writes d_grad_rhs and d_grad_fixed in device memory: it only
 * enqueues in the handle's stream and makes no host-synchronising call (the buffers of the per-cotangent form below are allocated at the first
 * call that needs them); d_G has to be complete in stream order.
 * Independence contract: the result of a cotangent does not depend on ncot, on its position in G, or on the other cotangents — it is bit for
 * bit the same; the same bits come back from run to run and from the host and the device form.  It is NOT promised to be bit-equal to
 * lexls_lse_solve_adjoint (the summation order differs): against that call, and against any reference, the contract is the tolerance one.
 * Errors, each returned before any device work and with every output left alone: LEXLS_ERR_INVALID for a null handle, a null G or a null
 * d_grad_rhs; LEXLS_ERR_INVALID for ncot == 0; LEXLS_ERR_INVALID when there is no kept factor; LEXLS_ERR_UNSUPPORTED when the factorization
 * ran with regularization_type != 0 and lexls_lse_set_adjoint_regularized_multi (below) is off, or the type or the variable factor is not served.
 * Kernel variant (lexls_lse_last_consumer_kernel), decided on the host from nVar and cap alone: "solve_adjoint_multi<64,staged>" — the
 * per-lane state and the staged factor fit one workgroup's 160 KiB of LDS; "solve_adjoint_multi<64,hbm>" — the state alone fits, the factor
 * is read where it is kept; "solve_adjoint<64> x K" — neither: the single-cotangent kernel once per cotangent. */
int lexls_lse_solve_adjoint_multi(lexls_lse_t h, const double *h_G, uint32_t ncot);
int lexls_lse_get_adjoint_multi(lexls_lse_t h, double *h_grad_rhs, double *h_grad_fixed);
int lexls_lse_solve_adjoint_multi_device(lexls_lse_t h, const double *d_G, uint32_t ncot, double *d_grad_rhs, double *d_grad_fixed);
/* on != 0: the three calls above serve a factor of regularization type 1, 3, 4, 5, 8 or 9 with variable_regularization_factor == 0 and return
 * M_reg^T g_c and N_reg^T g_c of the damped solve for every cotangent, with exactly the layouts, zero conventions, deferred-sync behaviour and
 * validity rule they have without regularization.  0 (the default): LEXLS_ERR_UNSUPPORTED after every regularized factorization, as before; the
 * message names this switch.  Independent of lexls_lse_set_adjoint_regularized (either, both or neither may be on).  Takes effect at the next
 * call; the kept factor stays valid.  LEXLS_ERR_INVALID for a null handle.  Types 2, 6 and 7 and a non-zero variable factor stay
 * LEXLS_ERR_UNSUPPORTED (the message names the condition); every refusal happens before any device work and leaves the outputs untouched.
 * lexls_lse_solve_adjoint_matrix* keeps refusing every regularized factorization.
 * The factors are read from the handle's device array AT THE TIME OF THE ADJOINT CALL, as in the single-cotangent call: a caller who rewrites
 * that array in place between the factorization and the call gets the adjoint of the rewritten factors, and no error is raised.
 * The independence contract above holds: a cotangent's bits do not depend on ncot, on its position in G or on its company; the same bits come
 * back run to run and from the host and the device form.  NOT promised bit-equal to lexls_lse_solve_adjoint: against it the contract is the
 * tolerance one.
 * One wavefront serves a problem and a tile of up to 64 cotangents, lane = cotangent; the grid is batch x tiles, and EVERY TILE REPEATS the
 * work of the problem (the rebuild of the null-space basis, the per-level snapshots, the formation of D and its Cholesky factorization): 65
 * cotangents cost two tiles' shared work.  Kernel variant (lexls_lse_last_consumer_kernel), decided on the host from nVar, cap and nObj alone:
 * "solve_adjoint_reg_multi<64,lds>" — the per-lane state and the problem's matrices fit one workgroup's 160 KiB of LDS;
 * "solve_adjoint_reg_multi<64,hbm>" — the state alone fits, the matrices sit in a work buffer of the handle (allocated at the first call that
 * needs it, and again when a call brings more tiles: that call of the device form is not enqueue-only); "solve_adjoint_reg<64,lds> x K" or
 * "solve_adjoint_reg<64,hbm> x K" — the state alone exceeds the limit: the single-cotangent kernel once per cotangent.
 * When it pays: the time of a call hardly depends on the number of live lanes of a tile — on 4096 IK problems (nVar 40, 5 x 12, type 1) 11.0 ms
 * for 1 cotangent, 11.4 ms for 40, 11.7 ms for 64 and 22.6 ms for 65 (MI355X), against 1.69 ms per call of
 * lexls_lse_solve_adjoint_device — so from about SEVEN cotangents per problem on it is faster than that many single-cotangent calls (5.9 times
 * at 40), and below that it is slower. */
int lexls_lse_set_adjoint_regularized_multi(lexls_lse_t h, int on);

/* Gradient of the solve with respect to the MATRIX A (and, with it, the right-hand sides): the derivative the calls above do not give.  x is
 * not continuous in A where a rank changes, so the derivative exists for RANK-STABLE problems only, and the call says per problem whether it
 * returned one.
 * Rank-stability rule, as the kernel evaluates it: a problem with every variable fixed is rank-stable; any other problem is rank-stable when
 * rank_k == min(dim_k, nVar - Fc_k) for every level k, with Fc_k the first column of level k (fixed variables included) and
 * min(dim_k, nVar - Fc_k) = 0 where Fc_k >= nVar — every level took all the rank it could; a level that finds the columns used up has rank 0
 * and passes.  Small perturbations of A move neither the ranks nor the pivots of such a problem.  For any other problem a generic perturbation
 * raises a rank and no derivative exists.
 * Formula: for a rank-stable problem the levels above k*, the last level of non-zero rank, act as equalities C x = d, level k* is a
 * least-squares objective min |E x - f|, the later levels do not touch x, free and fixed variables are further equalities.  With g = dloss/dx,
 * for every level k in the user's row and column order
 *     dloss/dA_k = - y_k x^T - lambda_k u^T,      dloss/db = y
 * x = the solution (lexls_lse_get_x order, fixed variables included); y = M^T g, the grad_rhs of lexls_lse_solve_adjoint; lambda = the
 * multipliers of level k* (its own rows hold its residual r = A_k* x - b_k*, the rows of the levels above hold nu with A_k*^T r + sum_j A_j^T
 * nu_j = 0 on the pivot variables, the rows below are zero: column k* of lexls_lse_multipliers); u = M y~ with y~ = y on the rows of level k*
 * and zero elsewhere, fixed values zero (u is zero on fixed and free variables).
 * Layouts: g is batch x nVar in the order of lexls_lse_get_x.  grad_lod is batch x (nVar + 1) x cap doubles, the layout of
 * lexls_lse_set_problem_host: entry (row i, column j) of problem b at b * (nVar + 1) * cap + j * cap + i; column j < nVar is the gradient of
 * column j of A, column nVar is y, the gradient of the right-hand side; rows behind the problem's own are zero.  differentiable is one byte
 * per problem: 1 = rank-stable, 0 = not — and where the flag is 0 the whole of that problem's grad_lod is exact zeros (the convention of
 * lexls_lsi_batch_solve_adjoint for instances that did not end PROBLEM_SOLVED).
 * The call needs the x of the current factor: lexls_lse_factorize_solve(keep_factor = 1), or lexls_lse_factorize + lexls_lse_solve.
 * lexls_lse_solve_adjoint_matrix copies h_g in, launches and keeps the results in buffers of the handle (allocated at the first call);
 * lexls_lse_get_adjoint_matrix copies them out, either output may be NULL; both follow lexls_lse_set_deferred_sync, and
 * lexls_lse_get_adjoint_matrix answers only while the results belong to the current factor, as lexls_lse_get_adjoint does.
 * lexls_lse_solve_adjoint_matrix_device reads d_g and writes d_grad_lod and d_differentiable (NULL: not wanted; d_grad_lod may not be NULL) in
 * device memory: it only enqueues in the handle's stream and makes no host-synchronising call (its work buffers are allocated at the first
 * call).  What lexls_lse_get_multipliers, lexls_lse_get_v, lexls_lse_get_lambda and lexls_lse_get_sensitivity answer is not changed by these
 * calls.
 * Tolerance contract (no reference arithmetic exists); no atomics, the same bits from run to run and from the host and the device form.
 * Errors, each returned before any device work and with every output left alone: LEXLS_ERR_INVALID for a null handle, a null g or a null
 * d_grad_lod; LEXLS_ERR_INVALID when there is no kept factor; LEXLS_ERR_INVALID when no x belongs to the current factor (lexls_lse_factorize
 * alone, or a least-norm solve); LEXLS_ERR_UNSUPPORTED when the factorization ran with regularization_type != 0
 * (every type: the single-cotangent call lexls_lse_solve_adjoint serves types 1, 3, 4, 5, 8 and 9, for the right-hand sides only).
 * Kernel variant: "solve_adjoint_matrix<64>" (lexls_lse_last_consumer_kernel). */
int lexls_lse_solve_adjoint_matrix(lexls_lse_t h, const double *h_g);
int lexls_lse_get_adjoint_matrix(lexls_lse_t h, double *h_grad_lod, uint8_t *h_differentiable);
int lexls_lse_solve_adjoint_matrix_device(lexls_lse_t h, const double *d_g, double *d_grad_lod, uint8_t *d_differentiable);

/* FORWARD-MODE tangents of the solve with respect to its data: how x moves along ntan directions d[A | b] (and dx_fixed) per problem, in one
 * pass over the directions and two over the kept factor — the transpose of lexls_lse_solve_adjoint_matrix, which needs nVar calls on unit
 * cotangents for the same quantity.  It exists where that gradient exists: for the RANK-STABLE problems of the rule above.
 * Formula, in the symbols above (M the solve map x = M b + N x_fixed, k* the last level of non-zero rank, E_k* = keep the rows of level k*,
 * lambda the multipliers of level k*), signs fixed against the dense KKT solve (tests/tangent_cases.py):
 *     dx = M [ (db - dA x - A_fixed dx_fixed) - E_k* M^T (dA^T lambda) ]  on the pivot variables,
 *     dx = dx_fixed on the fixed variables,  dx = 0 on the free variables (beyond the total rank).
 * Layouts: dlod is ntan x batch x (nVar + 1) x cap doubles, direction c of problem b in the layout of lexls_lse_set_problem_host (what grad_lod
 * has): entry (row i, column j) at ((c * batch + b) * (nVar + 1) + j) * cap + i, column nVar = db.  Entries of rows behind a problem's own
 * dimensions are never read (a NaN there does not reach dx).  dfixed is ntan x batch x nVar in the layout of grad_fixed of
 * lexls_lse_solve_adjoint: slot j < nfixed is the tangent of the j-th fixed value; NULL = zeros; the slots from nfixed on are never read.  dx is
 * ntan x batch x nVar in the variable order of lexls_lse_get_x.  differentiable is one byte per problem, the bits
 * lexls_lse_solve_adjoint_matrix writes; a problem with flag 0 gets exact zeros in all its rows of dx.
 * The call needs what lexls_lse_solve_adjoint_matrix needs: a kept, unregularized factor and the x that belongs to it.
 * lexls_lse_solve_tangent copies the directions in, launches and keeps the results in buffers of the handle (made for the largest ntan so far);
 * lexls_lse_get_tangent copies them out (ntan x batch x nVar for the ntan of that call, and the flags; either output may be NULL); both follow
 * lexls_lse_set_deferred_sync, and lexls_lse_get_tangent answers only while the results belong to the current factor.
 * lexls_lse_solve_tangent_device reads d_dlod and d_dfixed (NULL: zeros) and writes d_dx and d_differentiable (NULL: not wanted) in device
 * memory: it only enqueues in the handle's stream and makes no host-synchronising call (its work buffers are allocated at the first call and
 * whenever ntan exceeds every earlier one).  What lexls_lse_get_multipliers, lexls_lse_get_v, lexls_lse_get_lambda and
 * lexls_lse_get_sensitivity answer is not changed by these calls.
 * Independence contract: for ntan >= 2 the tangent of a direction does not depend on ntan, on its position or on the other directions, bit for
 * bit (one lane per direction, no cross-lane sums); the same bits come back from run to run and from the host and the device form.  ntan == 1
 * computes M^T (dA^T lambda) with the single-cotangent kernel, whose sums are ordered differently: between ntan == 1 and ntan >= 2, and against
 * any reference, the contract is the tolerance one.  No atomics.
 * Errors, each returned before any device work and with every output left alone: LEXLS_ERR_INVALID for a null handle, a null dlod, a null
 * d_dx, ntan == 0 or ntan > 65535; LEXLS_ERR_INVALID when there is no kept factor or no x belongs to it; LEXLS_ERR_UNSUPPORTED when the
 * factorization ran with regularization_type != 0.
 * Kernel variant (lexls_lse_last_consumer_kernel): "solve_tangent<64,staged>", "solve_tangent<64,lds>" or "solve_tangent<64,work>" — where the
 * per-direction vectors of the solve map live, decided from nVar, cap and nObj alone. */
int lexls_lse_solve_tangent(lexls_lse_t h, const double *h_dlod, const double *h_dfixed, uint32_t ntan);
int lexls_lse_get_tangent(lexls_lse_t h, double *h_dx, uint8_t *h_differentiable);
int lexls_lse_solve_tangent_device(lexls_lse_t h, const double *d_dlod, const double *d_dfixed, uint32_t ntan, double *d_dx, uint8_t *d_differentiable);

/* NEW RIGHT-HAND SIDES on the kept factor: the nrhs solutions x = M rhs + N fixed of every problem for the matrix that was factorized, without
 * factorizing again.  factorize() chooses pivots and ranks from A alone, so x is exactly affine in b and in the fixed values; the same holds
 * after a damped factorization of type 1, 3, 4, 5, 8 or 9 with constant factors (the regularization settings of the factorization stay).
 * Column c of problem b is the x lexls_lse_factorize_solve returns for that problem with its right-hand-side column replaced by rhs[c, b] and
 * its fixed values by fixed[c, b] — within the tolerance contract (no reference arithmetic exists for this path).  With the handle's own b and
 * fixed = NULL the result equals lexls_lse_get_x within that tolerance.
 * Layouts: rhs is nrhs x batch x cap, right-hand side c of problem b in LOD row order (the order of grad_rhs of lexls_lse_solve_adjoint); rows
 * behind a problem's own dimensions are never read (a NaN there reaches nothing).  fixed is nrhs x batch x nVar, slot j < nfixed the j-th fixed
 * value (as dfixed of lexls_lse_solve_tangent); NULL = the fixed values the handle holds; slots from nfixed on are never read.  x is nrhs x batch
 * x nVar in the order of lexls_lse_get_x: fixed variables carry their value, variables beyond the total rank what lexls_lse_solve leaves there
 * (zero).
 * Served: every problem of every kept factor from every producer (rank-deficient problems and problems with every variable fixed too: there is
 * no per-problem flag), plain and damped (types 1, 3, 4, 5, 8, 9), behind no switch.  No x of the current factor is needed: lexls_lse_factorize
 * alone is enough.
 * lexls_lse_solve_rhs copies the inputs in, launches and keeps the results in buffers of the handle (made for the largest nrhs so far);
 * lexls_lse_get_solve_rhs copies them out (nrhs x batch x nVar for the nrhs of that call); both follow lexls_lse_set_deferred_sync, and
 * lexls_lse_get_solve_rhs answers only while the results belong to the current factor.  lexls_lse_solve_rhs_device reads d_rhs and d_fixed
 * (NULL: the handle's) and writes d_x in device memory: it only enqueues in the handle's stream and makes no host-synchronising call (its work
 * buffer is allocated at the first call and whenever nrhs exceeds every earlier one).  What lexls_lse_get_x, _get_v, _get_lambda,
 * _get_multipliers, _get_sensitivity and _get_adjoint* answer is not changed by these calls.
 * Independence contract: for nrhs >= 2 the solution of a right-hand side does not depend on nrhs, on its position or on its company, bit for bit
 * (one lane per right-hand side, no cross-lane sums); the same bits come back from run to run and from the host and the device form.  On a plain
 * factor nrhs == 1 takes the single-vector kernel, whose sums are ordered differently: between nrhs == 1 and nrhs >= 2 the contract is the
 * tolerance one.  No atomics.
 * Errors, each returned before any device work and with every output left alone: LEXLS_ERR_INVALID for a null handle, a null rhs, a null d_x,
 * nrhs == 0 or nrhs > 65535, or no kept factor; LEXLS_ERR_UNSUPPORTED after a factorization with regularization_type 2, 6 or 7 or with
 * variable_regularization_factor != 0 (x is not an affine map of b there; the message names the condition).
 * Kernel variant (lexls_lse_last_consumer_kernel): plain "solve_rhs<64,single>" (nrhs == 1), "solve_rhs<64,staged>", "solve_rhs<64,lds>" or
 * "solve_rhs<64,work>"; damped "solve_rhs_reg<64,lds>", "solve_rhs_reg<64,hbm>" or "solve_rhs_reg<64,work>" — where the per-right-hand-side
 * vectors and the problem's matrices live, decided from nVar, cap and nObj alone.
 * Cost: a call costs about the same for 1 as for 64 right-hand sides (one wavefront per problem and tile of 64, lane = right-hand side).  On
 * the IK shape it is cheaper than refactorizing [A | b_new] from about 12 right-hand sides on for a plain factor, and only from
 * about 16 on for a damped one, where a single right-hand side costs as much as some 16 damped factorizations: below that, refactorize. */
int lexls_lse_solve_rhs(lexls_lse_t h, const double *h_rhs, const double *h_fixed, uint32_t nrhs);
int lexls_lse_get_solve_rhs(lexls_lse_t h, double *h_x);
int lexls_lse_solve_rhs_device(lexls_lse_t h, const double *d_rhs, const double *d_fixed, uint32_t nrhs, double *d_x);

/* RESIDUALS OF NEW RIGHT-HAND SIDES on the kept factor: what ranks the nrhs candidates of lexls_lse_solve_rhs — the residual v of every priority
 * level and its squared norm — without factorizing again and without a second copy of A (the factor overwrote it).
 * Inputs: rhs and fixed exactly as for lexls_lse_solve_rhs (nrhs x batch x cap; nrhs x batch x nVar, NULL = the handle's fixed values; rows and
 * slots behind a problem's own dimensions are never read).
 * v is nrhs x batch x cap in LOD row order: v[c, b, :] is what lexls_lse_residual followed by lexls_lse_get_v returns for problem b with its
 * right-hand-side column replaced by rhs[c, b] and its fixed values by fixed[c, b] — get_v() of the reference (lexlse.h:1560-1582), A x - b
 * recovered through Q — within the tolerance contract; rows behind the problem's dimensions are written as 0.  With the handle's own b and
 * fixed = NULL it equals lexls_lse_get_v within that tolerance.
 * cost is nrhs x batch x nObj: cost[c, b, k] = the sum of squares of level k's rows of v[c, b], one ordered fma chain in row order by the lane
 * that owns right-hand side c.  A level with rank == dim has its rows of v and its cost equal to 0.0 exactly (a zero head, nothing to push
 * through Q: the reference's behaviour).
 * d_x (device form), when non-NULL, receives the x of lexls_lse_solve_rhs_device for the same inputs, bit for bit: one call serves a caller who
 * wants both, and the forward pass runs once (nrhs == 1: x comes from the single-vector kernel, as there).
 * Served: every problem of every kept, UNDAMPED factor from every producer, rank-deficient problems and problems with every variable fixed
 * included.  After a factorization with regularization_type != 0: LEXLS_ERR_UNSUPPORTED (get_v's formula is the residual of the undamped basic
 * solution).  No x of the current factor is needed.
 * lexls_lse_residual_rhs copies the inputs in, launches and keeps v and cost in buffers of the handle (made for the largest nrhs so far);
 * lexls_lse_get_residual_rhs copies them out (either pointer may be NULL, not both) and answers only while they belong to the current factor;
 * both follow lexls_lse_set_deferred_sync.  lexls_lse_residual_rhs_device reads and writes device memory (any of d_x, d_v, d_cost may be NULL,
 * not all three), only enqueues in the handle's stream and makes no host-synchronising call (the work buffer, shared with
 * lexls_lse_solve_rhs_device, is allocated at the first call and whenever nrhs exceeds every earlier one).  What lexls_lse_get_x, _get_v,
 * _get_lambda, _get_multipliers, _get_solve_rhs and _get_adjoint* answer is not changed by these calls.
 * Independence contract: v and cost of a right-hand side do not depend on nrhs, on its position or on its company, bit for bit (one lane per
 * right-hand side, no cross-lane sums, no atomics); the same bits come back from run to run and from the host and the device form.
 * Errors, each returned before any device work and with every output left alone: LEXLS_ERR_INVALID for a null handle, a null rhs, every output
 * null, nrhs == 0 or nrhs > 65535, or no kept factor; LEXLS_ERR_UNSUPPORTED after a damped factorization (the message names the condition).
 * Kernel variant (lexls_lse_last_consumer_kernel): "residual_rhs<64,staged>", "residual_rhs<64,lds>" or "residual_rhs<64,work>" — the placement
 * rule of lexls_lse_solve_rhs, from nVar, cap and nObj alone.  Cost: DESIGN.md 5.15. */
int lexls_lse_residual_rhs(lexls_lse_t h, const double *h_rhs, const double *h_fixed, uint32_t nrhs);
int lexls_lse_get_residual_rhs(lexls_lse_t h, double *h_v, double *h_cost);
int lexls_lse_residual_rhs_device(lexls_lse_t h, const double *d_rhs, const double *d_fixed, uint32_t nrhs, double *d_x, double *d_v, double *d_cost);

/* ---- results (synchronise the stream, then D2H) ------------------------------------------------- */
int lexls_lse_get_x(lexls_lse_t h, double *h_x);                    /* get_x()      lexlse.h:1587 */
int lexls_lse_get_factor(lexls_lse_t h, double *h_lod);             /* get_lexqr()  lexlse.h:1626 */
int lexls_lse_get_hh_scalars(lexls_lse_t h, double *h_hh);
int lexls_lse_get_permutation(lexls_lse_t h, uint32_t *h_perm);
int lexls_lse_get_ranks(lexls_lse_t h, uint32_t *h_rank, uint32_t *h_first_col, uint32_t *h_total_rank); /* getRank/getTotalRank :1503,:1603 */
int lexls_lse_get_v(lexls_lse_t h, double *h_v);                    /* get_v()      lexlse.h:1560 */
/* replaces get_X_mu() / get_X_mu_rhs() / get_residual_mu() (lexlse.h:1636-1650), filled with regularization type 7 only: h_x_mu and
 * h_x_mu_rhs are batch x nObj x nVar (column k of the reference's nVar x nObj matrix is contiguous), h_residual_mu is batch x cap;
 * NULL = not wanted.  X_mu_rhs columns are written by lexls_lse_sensitivity (initialize_rhs, :1921-1959). */
int lexls_lse_get_mu(lexls_lse_t h, double *h_x_mu, double *h_x_mu_rhs, double *h_residual_mu);
int lexls_lse_get_lambda(lexls_lse_t h, double *h_lambda);          /* getWorkspace() after ObjectiveSensitivity, lexlse.h:1621 */
/* h_found_ctr_obj: batch x 3 int32 {found, CtrIndex2Remove, ObjIndex2Remove}; h_max_abs: batch */
int lexls_lse_get_sensitivity(lexls_lse_t h, int32_t *h_found_ctr_obj, double *h_max_abs);
int lexls_lse_get_wrong_sign(lexls_lse_t h, uint8_t *h_mask);    /* batch x (nVar + cap): the set of the last lexls_lse_sensitivity_collect call */
int lexls_lse_get_ctr_type(lexls_lse_t h, uint8_t *h_types);
int lexls_lse_get_fixed_type(lexls_lse_t h, uint8_t *h_types);   /* batch x nVar: activation types of the fixed variables incl. the CORRECT_SIGN_OF_LAMBDA marks (lexlse.h:866-987) */
/* raw device pointer of one of the handle's arrays (enum lexls_array), for zero-copy consumers */
int lexls_lse_device_ptr(lexls_lse_t h, int which, void **d_ptr);

/* name of the kernel variant the last factorize/factorize_solve call dispatched to (diagnostics) */
const char *lexls_lse_last_kernel(lexls_lse_t h);
/* name of the kernel variant that served the last post-factorization call (solve, residual, sensitivity / sensitivity_collect, multipliers,
 * solve_least_norm*), NUL-terminated into buf[0 .. len) and cut to len - 1 characters: "solve_generic<256>", "residual<64>",
 * "sensitivity_sweep<12>", "sensitivity<64,staged>", "sensitivity<64,hbm>", "multipliers_sweep<16>", "multipliers<per-objective>",
 * "leastnorm_2<64>", ...; "" after a factorization until one of them launches (a lexls_lse_solve the factorization kernel had answered
 * already launches nothing).  Written on the host by the launchers: diagnostics, no kernel and no launch depends on it */
int lexls_lse_last_consumer_kernel(lexls_lse_t h, char *buf, size_t len);
/* lqr_large<step-per-pivot,mfma> runs the pivots of a level of a SINGLE problem inside one launch (lqr_large.hip, fast_level_persist); a launch
 * whose bounded hand-offs ran out raises its abort flag, commits nothing, and the host redoes the level with a launch per pivot.  Of the last
 * factorization: *in_launch = levels the one-launch form committed, *redone = levels it gave up (both 0 on every other kernel, for a batch, under
 * LEXLS_LARGE_PERSIST=0 and where no form of the launch fits the device; LEXLS_LARGE_PERSIST=2 gives up on every level it is tried on).  Read on the host from
 * the flag the launcher reads anyway: diagnostics, no kernel and no launch depends on it */
int lexls_lse_last_large_levels(lexls_lse_t h, uint32_t *in_launch, uint32_t *redone);
/* lqr_wave<..,regularized> keeps the regularization routines' optional pieces in LDS as far as the launcher finds room for them
 * (wave_reg_lds_bytes, lexls_lds.h); what does not fit stays in the handle's scratch in HBM: same routines, same bits, other address space.
 * Of the last factorization: *window_order = order of the LDS window of the routines' work matrix (a level whose normal equations have a
 * larger order works in HBM; 0: no window), *basis_in_lds = 1 when the accumulated null-space basis was kept in LDS (both 0 on every
 * other kernel — the generic kernel keeps all of it in HBM — and without regularization).  Stored on the host by the launcher, the value it
 * passed to the launch: diagnostics, no kernel and no launch depends on it */
int lexls_lse_last_reg_placement(lexls_lse_t h, uint32_t *window_order, uint32_t *basis_in_lds);
/* Kernel policy — which CONTRACT a solve is held to, and which kernel family serves it.
 *   Contracts: (B) bit-identical to the arithmetic contract of oracle/lexlse_oracle.h (pivots, ranks, Householder scalars, factor, x, multipliers);
 *              (T) BASELINE north_star's: column permutation, ranks and first columns exact, x (and factor MAGNITUDES) within 1e-10
 *                  (relative to max(1, |x|_inf)) — on problems whose own solution is determined that well.  An ill-conditioned problem
 *                  (tiny pivots above the rank tolerance, rows / columns scaled over many decades), whose x moves by more than ~1e-11 when
 *                  its DATA move by one ulp, is solved to a small multiple of that sensitivity instead (scripts/soak_qtol.py: 21 k
 *                  random batches, 92 such problems beyond 1e-10, at most 20 x their one-ulp sensitivity — 47 x once levels of eight rows
 *                  joined the soak, 91 x on lqr_mfma's soak; the soaks' bound is 100 x, a random one-ulp perturbation being a LOWER
 *                  estimate of what rounding does to such a problem —; pivots and ranks exact in all.  Policy 10 opens hierarchies of
 *                  SHORT levels, where badly scaled data have exceeded that multiple: see policy 10 below).
 *                  PIVOT RULE under (T).  The reference takes the first maximum of the down-dated column norms (lexlse.h:205-206).  lqr_mfma compares
 *                  the norms by VALUE (whole doubles; equal values: the smallest position) — the reference's rule on this kernel's own norms.
 *                  lqr_qtol compares them in ONE max butterfly on a packed key whose low 12 mantissa bits carry the position: two candidates whose
 *                  norms agree in their upper 40 mantissa bits (relative difference below 2^-40 = 9.1e-13) are ordered BY POSITION, whatever their
 *                  last 12 bits say.  Exact ties (duplicated columns) are ordered as the reference orders them by either kernel; norms that differ by
 *                  1e-11 relative or more are ordered by value by both (tests/test_gpu_qtol.py, tests/test_gpu_mfma.py: near-tie cases).
 *   policy 0 = automatic dispatch.  (T) for x-only solves whose levels ALL have 12 rows (or ALL 8: round 4), no fixed variables, no regularization, n <= 40 (the IK shape of
 *              BASELINE configs[2]/[3] and its smaller relatives):
 *              lqr_qtol, the bench kernel — and for problems beyond one CU's LDS (the step-per-pivot path with the trailing update on the matrix
 *              cores; there the reflector of a row that exactly repeats a row of an earlier level may come out with the opposite SIGN — that row of R
 *              and its essential part are negated, x and everything else agree: consumers of get_lexqr / hh scalars that need sign parity with the
 *              ordered-chain arithmetic ask for policy 5).  (B) for everything else: with the factor kept the register-resident wave kernel while
 *              the batch fits one round of it, beyond that the four-per-wavefront kernel's factor-keeping form (the left-looking wave kernel
 *              where that does not fit); x-only solves of other small shapes the four-per-wavefront kernel.  LEXLS_QTOL=0 in the environment keeps
 *              every small-shape solve on (B).
 *   1 = only the generic one-workgroup-per-problem kernel (B);  2 = automatic, but never the left-looking / four-per-wavefront kernels (B);
 *   3 = the left-looking wave kernel whenever the shape allows it, whatever the batch size (B);
 *   4 = the bit-exact four-problems-per-wavefront kernel whenever the shape allows it (x-only solves; else as 3) (B);
 *   5 = automatic with (B) everywhere: small shapes as under LEXLS_QTOL=0, large problems on the bit-exact multi-launch path (ordered chains, two
 *       launches per pivot) — the policy for factor / sign parity;
 *   6 = the tolerance-contract kernel lqr_qtol wherever it serves (T), else as 0;
 *   7 = the matrix-core tolerance-contract kernel lqr_mfma (lexls_amd/csrc/lqr_mfma_impl.h: two problems per wavefront, two wavefronts per SIMD, the
 *       Gauss step of lexlse.h:431-471 on v_mfma_f64_16x16x4_f64, finished levels kept in reduced form) wherever it serves (T) — x-only solves
 *       whose levels all have 12 rows, n + 1 <= 48, no fixed variables / regularization, two workgroups' LDS slices per CU (n = 40: up to 5 levels) —
 *       else as 6;  8 = the same kernel with one problem per wavefront (four wavefronts per SIMD);  9 = with four problems per wavefront (the IK
 *       shape only).  Automatic dispatch (0) takes lqr_qtol first — the faster one on MI355X (41 us against 57 us per 4096 IK problems) — and
 *       lqr_mfma for the shapes lqr_qtol's slices do not hold.
 *   10 = as 6, and additionally lqr_qtol's RAGGED instantiations (T) for x-only solves whose levels have AT MOST 12 rows each — per-problem
 *       dimensions (lexls_lse_set_obj_dim(..., per_problem = 1)), any mix, empty levels included — under lqr_qtol's other conditions (no fixed
 *       variables, no regularization, factor not kept, <= 8 levels, n <= 40 in practice).  A batch whose levels all have 12 (or all 8) rows takes
 *       the same kernel as under 6; what the ragged form does not serve goes where 6 sends it.  Opt-in: policy 0 keeps such batches on (B).
 *       Contract (T), same 2^-40 position window of the pivot rule: a level of d rows is factorized as that level with zero rows appended,
 *       which changes neither pivots nor x (tests/test_ragged_padding_oracle.py); x is bit-identical to lqr_qtol's on the zero-padded problem.
 *       MEASURED on hierarchies of short levels (scripts/soak_qtol_ragged.py, 13 k random batches, pivots and ranks exact in all): on data whose
 *       rows are scaled over four and columns over six decades, 2 problems (levels of 2 / 7 / 3 / 2 and of <= 12 rows, n = 14 and 11) came out at
 *       1.12e-10 and 1.23e-10 — just beyond 1e-10 although their one-ulp sensitivity is 1.1e-13 and 3.0e-14 (990 x and 4,147 x: beyond the
 *       100 x the soaks allow; the uniform kernels' largest is 47 x).  It is lqr_qtol's arithmetic on such levels, not the ragged loads (same
 *       bits as the uniform kernel on the padded problems).  A caller with badly scaled data and short levels should not rely on 1e-10 under
 *       policy 10; well-scaled data keep it (every case of tests/test_gpu_qtol_ragged.py).  With the accuracy guard on, a ragged batch takes the bit-exact
 *       kernel of its shape (status 0): there is no estimating ragged instantiation.
 *   Policy 0 is therefore NOT bit-exact for those x-only solves; a caller that needs (B) everywhere sets policy 5 (per handle) or runs under
 *   LEXLS_QTOL=0 (whole process; read at every factorization, so it may be changed between solves) — or switches the accuracy guard on below.
 *   ACCURACY GUARD (lexls_lse_set_accuracy_guard, off by default).  With the guard on, a solve that would run on lqr_qtol (policies 0 and 6; uniform batches under 10) runs on
 *   its estimating instantiation, which also writes per problem an estimate of how far it can vouch for its (T) answer: the maximum over the
 *   pivots of |pivot column in its level's raw rows| / |R_jj| (cancellation in the factorization).  A solve that would run on another (T) kernel
 *   (lqr_mfma: policy 0 for shapes lqr_qtol does not hold, policies 7 / 8 / 9; the step-per-pivot large path) takes the bit-exact kernel for the
 *   shape instead.  CONTRACT of mode 2: every problem is either solved under (B), or under (T) with an estimate below the threshold — a flagged
 *   problem is re-solved in the same stream by the bit-exact four-per-wavefront kernel (the one policy 4 takes), so its x, ranks, first columns
 *   and permutation are bit-identical to the oracle.  Mode 1 only reports.  The default threshold (64) separates, with about five times room
 *   either way, well-conditioned IK problems (estimates up to 13) from every problem whose x moves by more than 1e-11 under one-ulp changes of its
 *   data on the calibration sets (estimates from 421 on: scripts/calibrate_guard.py); it flags every badly scaled problem too. */
int lexls_lse_set_kernel_policy(lexls_lse_t h, int policy);

/* mode 0: off (default, today's behaviour). 1: report only. 2: report + re-solve flagged problems under (B).
 * threshold <= 0: the calibrated default.  Takes effect at the next factorization; the guard never syncs the stream nor copies to the host
 * inside a solve (deferred sync keeps working). */
int lexls_lse_set_accuracy_guard(lexls_lse_t h, int mode, double threshold);
/* per problem: estimate (double) and status (uint8): 0 solved under (B) by the kernel chosen,
 * 1 (T) and estimate below the threshold, 2 (T) flagged and not re-solved (mode 1),
 * 3 flagged and re-solved under (B) (mode 2).  *h_flagged = number of problems with status 2 or 3. Any pointer may be NULL.
 * Describes the last factorization; all zeros when it ran with the guard off.  Waits for the handle's stream (also under deferred sync).
 * Status 0 problems report estimate 0.
 * Under a skip mask (lexls_lse_set_skip) the report of a skipped problem is KEPT: estimate and status stay those of the factorization that
 * produced its results, on the estimating kernel and on a bit-exact plan alike, and mode 2 does not re-solve it (its input is not read).
 * The same guard mode and threshold are assumed from run to run: the status of a kept estimate is re-derived under the current ones. */
int lexls_lse_get_accuracy(lexls_lse_t h, double *h_estimate, uint8_t *h_status, uint32_t *h_flagged);

/* ---- prefix reuse ------------------------------------------------------------------------------
 * The reference refactorizes the whole hierarchy in every LexLSI iteration although one row of one level changed (README.md:14 "No update
 * mechanism ... each iteration of the solver performs a full decomposition"; the loop at lexlsi.h:1144-1172 calls factorize() on the whole
 * problem).  Here a factorization can pick up the previous one of the same handle: with
 *     lexls_lse_set_prefix_reuse(h, 1)
 * every factor-keeping factorization by the register-resident wave kernel (IK-sized problems: nVar + 1 <= 64 columns, <= 64 rows — the kernel of
 * a LexLSI stage; lexls_lse_prefix_reuse_ready(h) says whether the last one was) also leaves the position map after each level, and
 *     lexls_lse_set_resume_levels(h, levels[batch])
 * tells the NEXT factorization that, for problem b, levels 0 .. levels[b]-1 — their rows, dimensions and the fixed variables — are exactly
 * those of its previous factorization, which still sits in the factor buffer.  Those levels are read back instead of factorized (no pivot
 * search, no reflectors: the dependent chains that make up most of the kernel's time); their elimination of the rows from level levels[b] on is
 * redone with the same instructions on the same operands.  Factor, permutation, ranks, Householder scalars and x are IDENTICAL, bit for bit, to
 * a full factorization (tests/test_gpu_prefix_reuse.py).  levels[b] = 0: factorize everything.  The levels are consumed by that factorization.
 * The caller vouches for "unchanged": the kernel does not compare rows.  (A change of the rank tolerance is seen by the handle itself:
 * lexls_lse_set_tolerance drops the state and the levels set.)  Regularization, x-only solves and the other kernels ignore the request
 * (full factorization) and leave nothing to resume from. */
int lexls_lse_set_prefix_reuse(lexls_lse_t h, int enable);
int lexls_lse_prefix_reuse_ready(lexls_lse_t h);
int lexls_lse_set_resume_levels(lexls_lse_t h, const int32_t *h_levels);

/* ---- inequality problems: the reference's LexLSI active-set driver (lexlsi.h), kept on the host -------------
 * The driver is host C++ (include/lexls/lexlsi.h, same logic as the reference's lexlsi.h/objective.h/workingset.h);
 * every factorize / solve / ObjectiveSensitivity it issues goes to the HIP kernels above.  Call sequence = the
 * reference's MEX front end (interfaces/matlab-octave/lexlsi.cpp:527-625).
 *   h_dims[nObj]; h_types[nObj]: 0 general, 1 simple bounds (objective 0 only, typedefs.h:60-64);
 *   h_data: objectives back to back, column-major: general dim x (nVar+2) = [A lb ub], simple dim x 2 = [lb ub];
 *   h_var_index[dims[0]]: 0-based variable indices of a simple-bounds objective (else NULL);
 *   h_active_guess: sum(dims) ConstraintActivationType bytes or NULL; h_x0: nVar or NULL;
 *   h_params9: {max_number_of_factorizations, tol_linear_dependence, tol_wrong_sign_lambda, tol_correct_sign_lambda,
 *               tol_feasibility, cycling_handling_enabled, cycling_max_counter, cycling_relax_step,
 *               deactivate_first_wrong_sign} or NULL for the defaults of typedefs.h:268-294;
 *   h_params of the entries that take nparams: nparams == 9 holds the above; 12 adds {regularization_type, variable_regularization_factor,
 *               max_number_of_CG_iterations}; 17 adds the hot-start options behind those, 0 / 1 each, in the order of typedefs.h:213-217:
 *               [12] modify_x_guess_enabled (0), [13] modify_type_active_enabled (0), [14] modify_type_inactive_enabled (0),
 *               [15] set_min_init_ctr_violation (1), [16] use_phase1_v0 (0) (defaults in brackets).  Every other count is LEXLS_ERR_INVALID.
 *               Slots 12 .. 15 are honoured by every entry, by the device's phase 1 (lexls_lsi_batch_run_device(_ex), lexls_lsi_batch_enqueue_device)
 *               in a setup kernel of their own; a run with the defaults launches what it always has.  use_phase1_v0 is served by every entry as well:
 *               on the device iteration 0 runs without a factorization (dx = 0, blocking test, no removal search) in place of the first stage.
 *               Without x0 every entry answers LEXLS_ERR_INVALID ("when use_phase1_v0 = true, x_guess has to be specified") before any device
 *               work.  A run that an entry refuses without the options is refused with them, with the same code.  Activation order: modify_type_* lets phase 1 activate and re-type constraints behind the list
 *               deactivate_first_wrong_sign walks; the reference leaves that list stale (its walk and its erase are then undefined).  Here the
 *               list is rebuilt behind phase 1: the entries still active with their type, in their order, then the constraints phase 1 activated,
 *               objective by objective in working-set order.  For modify_type_* with deactivate_first_wrong_sign this order is ours; for every
 *               other combination x, v, the active set and h_info6 are the reference's;
 *   outputs: h_x[nVar]; h_info6 = {status, iterations, activations, deactivations, factorizations, total_rank};
 *            h_active[sum(dims)] final working set; h_v[sum(dims)] constraint violations (either may be NULL). */
int lexls_lsi_solve(int device, uint32_t nVar, uint32_t nObj, const uint32_t *h_dims, const int32_t *h_types, const double *h_data,
                    const uint32_t *h_var_index, const uint8_t *h_active_guess, const double *h_x0, const double *h_params9, double *h_x,
                    int32_t *h_info6, uint8_t *h_active, double *h_v);
/* A batch of LexLSI problems of ONE structure (same nVar, dims, types; different data), advanced in LOCK STEP: every
 * active-set round issues one batched factorize+solve and one batched ObjectiveSensitivity per LexLSE level for all the
 * instances that need it (BASELINE configs[4]).  Arrays are the per-problem arrays of lexls_lsi_solve, back to back
 * (h_var_index: batch x dims[0]; h_active_guess / h_x0 may be NULL); h_rounds2 (may be NULL) receives
 * {factorize+solve stages, sensitivity stages} actually issued to the device.  The instances are split into g groups (default: 2 from 512
 * instances on, else 1; LEXLS_LSI_GROUPS=g overrides) that take turns: one group's stage runs on the GPU while the host advances the other
 * groups' active sets. */
int lexls_lsi_batch_solve(int device, uint32_t batch, uint32_t nVar, uint32_t nObj, const uint32_t *h_dims, const int32_t *h_types,
                          const double *h_data, const uint32_t *h_var_index, const uint8_t *h_active_guess, const double *h_x0,
                          const double *h_params9, double *h_x, int32_t *h_info6, uint8_t *h_active, double *h_v, int32_t *h_rounds2);
/* lexls_lsi_batch_solve with the regularization inputs of lexls_lsi_solve_ex: h_reg_factors = one factor per objective, shared by the batch,
 * or NULL; h_params with nparams == 9, 12 (+ regularization_type, variable_regularization_factor, max_number_of_CG_iterations) or 17 (+ the
 * hot-start options, see lexls_lsi_solve).
 * Regularized batches (every regularization_type but the experimental 7) run their active-set iterations resident on the device like plain ones,
 * on the REG instantiations of the register-resident l-QR where the shape has one ("How a run executes" below); type 7 and the other shapes
 * keep the host-driven lock-step stages, their factorizations on the generic kernel. */
int lexls_lsi_batch_solve_ex(int device, uint32_t batch, uint32_t nVar, uint32_t nObj, const uint32_t *h_dims, const int32_t *h_types,
                             const double *h_data, const uint32_t *h_var_index, const uint8_t *h_active_guess, const double *h_x0,
                             const double *h_reg_factors, const double *h_params, uint32_t nparams, double *h_x, int32_t *h_info6,
                             uint8_t *h_active, double *h_v, int32_t *h_rounds2);
/* lexls_lsi_batch_solve_ex plus the multipliers of every instance: h_lambda (batch x sum(dims) x nObj, layout of lexls_lsi_batch_get_lambda) or
 * NULL (= lexls_lsi_batch_solve_ex) */
int lexls_lsi_batch_solve_ex2(int device, uint32_t batch, uint32_t nVar, uint32_t nObj, const uint32_t *h_dims, const int32_t *h_types,
                              const double *h_data, const uint32_t *h_var_index, const uint8_t *h_active_guess, const double *h_x0,
                              const double *h_reg_factors, const double *h_params, uint32_t nparams, double *h_x, int32_t *h_info6,
                              uint8_t *h_active, double *h_v, int32_t *h_rounds2, double *h_lambda);
/* The same batch as an object that outlives one solve — the way the reference uses LexLSI (constructed and sized once, lexlsi.h:56-112, then
 * fed successive problems): lexls_lsi_batch_create makes the device buffers, pinned blocks, streams and the host worker pool for `batch`
 * problems of the structure (nVar, dims, types); every lexls_lsi_batch_run solves `batch` new problems of that structure (arguments as
 * lexls_lsi_batch_solve_ex).  lexls_lsi_batch_solve(_ex) = create + run + destroy; a serving loop saves the 6-8 ms of create per call. */
typedef struct lexls_lsi_batch_s *lexls_lsi_batch_t;
int lexls_lsi_batch_create(lexls_lsi_batch_t *out, int device, uint32_t batch, uint32_t nVar, uint32_t nObj, const uint32_t *h_dims, const int32_t *h_types);
int lexls_lsi_batch_run(lexls_lsi_batch_t b, const double *h_data, const uint32_t *h_var_index, const uint8_t *h_active_guess, const double *h_x0,
                        const double *h_v0 /* batch x sum(dims) initial residuals (set_v0, lexlsi.cpp:571-588) or NULL */, const double *h_reg_factors, const double *h_params, uint32_t nparams, double *h_x, int32_t *h_info6, uint8_t *h_active,
                        double *h_v, int32_t *h_rounds2);
/* lexls_lsi_batch_run for a caller whose problems are in device memory already (a simulator, a torch pipeline): the same arrays and layouts, in
 * memory of the batch's device — d_data (batch x per-instance data), d_var_index (batch x dims[0]; required with a simple-bounds objective 0, else
 * NULL), d_active_guess / d_x0 (may be NULL) in, d_x (required) and d_info6 / d_active / d_v (may be NULL) out.  It stands for these members of
 * lexls_lsi_batch_run: h_data, h_var_index, h_active_guess, h_x0, h_x, h_info6, h_active, h_v; h_v0 and h_rounds2 have no counterpart (initial
 * residuals are taken by lexls_lsi_batch_run_device_ex below; lexls_lsi_batch_stats has the stage counts).  Parameters and regularization factors stay host arrays.
 * The caller has finished writing the inputs before the call; the call returns when the outputs are complete (host-synchronous).  No constraint
 * data, state or result passes through host memory: the data is copied device-to-device into every group's resident copy (the caller's arrays
 * are never written, runs with cycling handling included), phase 1 is device work (below), a scatter kernel writes the results from the resident
 * slabs.  What does come back to the host: a fault word, the count of stopped instances, and after the run the working-set lists and counters
 * that lexls_lsi_batch_get_lambda / _get_cycling_counters / _stats / _last_kernel answer from, as after the equivalent lexls_lsi_batch_run.
 * Serves every run that is resident (next paragraph).  Everything else returns LEXLS_ERR_UNSUPPORTED before any device work and leaves the outputs
 * alone — LEXLS_LSI_RESIDENT=0, LEXLS_LSI_HOST_STAGING, regularization_type 7, cycling handling of a regularized run, shapes without a
 * register-resident kernel: there is no detour over the host.  An instance with lb > ub, variable indices that repeat or are not below nVar, or a
 * guess flag above 3 ends the call with LEXLS_ERR_INVALID before anything is solved; lexls_last_error() names the first such instance and the reason. */
int lexls_lsi_batch_run_device(lexls_lsi_batch_t b, const double *d_data, const uint32_t *d_var_index, const uint8_t *d_active_guess,
                               const double *d_x0, const double *h_reg_factors, const double *h_params, uint32_t nparams, double *d_x, int32_t *d_info6, uint8_t *d_active, double *d_v);
/* lexls_lsi_batch_run_device with the rest of a warm start and of the results in device memory, for a closed loop on the device: solve, perturb
 * the data there, solve again from active / x / v of the previous answer.  lexls_lsi_batch_run_device itself is unchanged; with d_v0, d_lambda and
 * d_cycling_counts all NULL this call IS that one (the old entry point calls this one with the three NULL).  The three may be given in any combination.
 * d_v0: batch x sum(dims) initial residuals, the layout of h_v0 of lexls_lsi_batch_run — the reference's set_v0 per objective (lexlsi.cpp:571-588).
 *   Together with d_x0 every objective's v is the given vector as it stands: A x0 is still formed, the guess is activated as given, and neither
 *   formInitialWorkingSet nor initialize_v0 is run (Objective::phase1, objective.h:226-236) — a branch of the phase-1 setup kernel that reads the
 *   caller's array where it lies; nothing of v0 passes through host memory and the array is never written.  d_v0 without d_x0 is disregarded, as
 *   the reference does (lexlsi.h:695-701): the run is the one without v0.  The reference's warning is not printed (warnings are not reproduced on
 *   this path), and its "partially specified" case cannot arise: one array covers all objectives.
 * d_lambda: batch x sum(dims) x nObj doubles, the layout of lexls_lsi_batch_get_lambda — the multipliers of THIS run, written by the scatter kernel
 *   that puts them into the user's order straight into the caller's device array (no host copy).  Same conditions as lexls_lsi_batch_get_lambda:
 *   for a run after which that call would answer LEXLS_ERR_UNSUPPORTED — cycling handling enabled, regularization_type != 0, more than 65535
 *   constraints per instance — this call returns LEXLS_ERR_UNSUPPORTED when d_lambda is non-NULL, before any device work, every output left alone
 *   (the rule of lexls_lsi_batch_run_device: no detour).  A later lexls_lsi_batch_get_lambda on the batch still answers, with the same bits.
 * d_cycling_counts: `batch` uint32, what lexls_lsi_batch_get_cycling_counters returns, written by the result scatter kernel; zeros after a run
 *   without cycling handling.
 * Otherwise as lexls_lsi_batch_run_device: host-synchronous, LEXLS_ERR_UNSUPPORTED for every run that is not resident, LEXLS_ERR_INVALID for input
 * faults.  lexls_lsi_batch_run keeps its behaviour: LEXLS_LSI_DEVICE_PHASE1=1 still changes nothing when h_v0 is given. */
int lexls_lsi_batch_run_device_ex(lexls_lsi_batch_t b, const double *d_data, const uint32_t *d_var_index, const uint8_t *d_active_guess,
                                  const double *d_x0, const double *d_v0, const double *h_reg_factors, const double *h_params, uint32_t nparams,
                                  double *d_x, int32_t *d_info6, uint8_t *d_active, double *d_v,
                                  double *d_lambda, uint32_t *d_cycling_counts);
/* lexls_lsi_batch_run_device_ex as work in a stream: the same arguments and layouts, the same bits in the outputs, but the call only ENQUEUES the run
 * in hip_stream (a hipStream_t; NULL: the default stream) and returns.  It makes no host-synchronising HIP call, and no hipMalloc / hipFree once the
 * batch has served one enqueue with the same options (the first such call may allocate).  What is enqueued is what the synchronous call enqueues —
 * the device-to-device copy of the data, lsi_phase1_setup_kernel, the first stage, lsi_phase1_finish_kernel, the persistent launch of every remaining
 * iteration, lsi_result_scatter, and with d_lambda the multipliers' stage — in the stream of the batch's group, which forks from hip_stream and joins it
 * again by events.  The caller's inputs need only be complete in stream order; work enqueued later in hip_stream sees complete outputs.  The host
 * arrays (h_params, h_reg_factors, host factors of lexls_lsi_batch_set_instance_regularization) are read during the call.
 * Input errors are handled on the device: behind the setup kernels a small kernel reads the fault word (instance * 8 + code; 1 lb > ub, 2 variable
 * index not below nVar, 3 repeated variable index, 4 guess flag above 3) and, if it is set, stops every instance of the run by the mechanism that
 * stops a finished one — no later kernel touches the run's data and every output array is left as it was.  d_status (one word in device memory, or
 * NULL) receives the word, 0xffffffff for a good run; the scatter step writes it on both outcomes.
 * Served: the runs lexls_lsi_batch_run_device_ex serves whose resident iterations are ONE persistent launch (lexls_lsi_batch_last_kernel names
 * lsi_fused<...> after the synchronous call): plain and regularized runs (types 1..6, 8, 9), deactivate_first_wrong_sign, cycling handling of an
 * unregularized run, host or device per-instance factors, the working-set log.  Everything else returns LEXLS_ERR_UNSUPPORTED before any device work,
 * every output left alone — what lexls_lsi_batch_run_device_ex refuses, LEXLS_LSI_NO_FUSED=1, a shape without a persistent instantiation or whose
 * launch does not get its LDS, d_lambda where lexls_lsi_batch_get_lambda would refuse; this is decided on the host from the shape, not by trying the
 * launch.  A batch split into several groups (only LEXLS_LSI_GROUPS does that to a batch whose runs are resident) is not served either.
 * d_lambda: the final equality problems are formed by a kernel from the working sets where they live (lsi_lambda_form_kernel), then gathered, factorized
 * and swept as lexls_lsi_batch_get_lambda does; with an input error the stage runs on empty problems and the array is left as it was.
 * Between an enqueue and its finish lexls_lsi_batch_run*, _get_lambda, _get_cycling_counters, _stats and _get_working_set_log return LEXLS_ERR_INVALID.
 * A further enqueue without a finish in between is allowed — the closed loop: solve, perturb on the device, solve again — and ordered behind the
 * previous one when it goes into the same stream (host per-instance factors may not change between the two).
 * Capture: after one uncaptured enqueue + finish with the same options, an enqueue on a capturing stream (hipStreamBeginCapture, torch.cuda.graph)
 * is captured whole; a replay reads and writes the same device arrays with the parameters of the capturing call.  While a captured graph of a batch is
 * in use, the only other call on that batch is lexls_lsi_batch_finish.  The library sets no queue count.
 * A call that fails after it has begun to enqueue (LEXLS_ERR_HIP, an internal error) may leave part of a run in hip_stream; the batch then counts as
 * enqueued: lexls_lsi_batch_finish brings it back to order. */
int lexls_lsi_batch_enqueue_device(lexls_lsi_batch_t b, void *hip_stream, const double *d_data, const uint32_t *d_var_index, const uint8_t *d_active_guess,
                                   const double *d_x0, const double *d_v0, const double *h_reg_factors, const double *h_params, uint32_t nparams,
                                   double *d_x, int32_t *d_info6, uint8_t *d_active, double *d_v, double *d_lambda, uint32_t *d_cycling_counts,
                                   uint32_t *d_status);
/* Waits for hip_stream (NULL: the stream of the last lexls_lsi_batch_enqueue_device), then brings back what lexls_lsi_batch_run_device_ex downloads before
 * it returns: the working-set lists and fixed bounds lexls_lsi_batch_get_lambda forms its problems from, cycling counts, iteration counters, the kernel
 * name.  After it lexls_lsi_batch_get_lambda, _get_cycling_counters, _stats, _last_kernel, _get_working_set_log and _working_set_log_device answer as
 * after the equivalent synchronous call.  LEXLS_ERR_INVALID when the run had an input error, lexls_last_error() naming the instance and the reason as
 * the synchronous call does; the batch then takes the next enqueue normally.  It answers for the LAST enqueue only: in a loop of several enqueues
 * behind one finish, an input error of an earlier step shows in that step's d_status alone (and in its untouched outputs).  After a replay of a captured enqueue, lexls_lsi_batch_finish(b,
 * replay_stream) answers for that replay. */
int lexls_lsi_batch_finish(lexls_lsi_batch_t b, void *hip_stream);
/* Regularization factors of its own for every instance of the batch, in place of the one shared vector h_reg_factors of the runs: `factors` holds
 * batch x nObj doubles, instance-major — the layout of h_reg_factors repeated per instance; for objective k, instance b takes
 * factors[b * nObj + k] where the shared vector would have given h_reg_factors[k] (the entry of a simple-bounds objective 0 is ignored, as it is
 * there).  This is what N separate LexLSI objects with N factor sets compute (setRegularizationFactor per objective, lexlsi.cpp:527-625).
 * in_device_memory == 0: the array is copied at the call and may be freed.  in_device_memory == 1: the POINTER is kept — memory of the batch's
 * device, alive until the setting is cleared or the batch destroyed — and read in the groups' streams at the start of every run, so a closed
 * loop may rewrite the array in place between two runs (the caller's writes are complete before the run is called, as for every d_* input).
 * factors == NULL clears the setting: the batch behaves as if this call had never been made.
 * While the setting holds it serves every run of the object — lexls_lsi_batch_run, lexls_lsi_batch_run_device, lexls_lsi_batch_run_device_ex —
 * and such a run passes h_reg_factors == NULL (no rule says which of two sources would win).  A run with regularization_type 0 ignores the
 * setting as it ignores h_reg_factors.  The one-shot calls lexls_lsi_batch_solve* make their own batch object: shared factors only.
 * What it does on each path of "How a run executes" below:
 *   resident runs (persistent launch and lock-step stages alike): every group's regularization block is filled per instance — row lo + i of
 *     the array is row i of the group whose first instance is lo, LexLSE level k takes the entry of objective k + 1 when objective 0 holds simple
 *     bounds, else of objective k.  Host factors go through the block's staging copy, once per run; device factors are moved by one small
 *     kernel (lsi_instance_factors_kernel, one thread per instance and level) in the group's stream before the run's first stage, and are
 *     never copied to the host.  The kernels are those of a shared-factor run of the same type (lexls_lsi_batch_last_kernel names the same):
 *     the regularized instantiations have always indexed the factors by problem;
 *   phase 1 on the host (lexls_lsi_batch_run by default), host factors: the host LexLSI object of instance b gets row b.  With DEVICE factors
 *     lexls_lsi_batch_run makes phase 1 device work, as if LEXLS_LSI_DEVICE_PHASE1=1 were set for that run — no host object may read the array —
 *     and, as that path takes no h_v0, a run that gives h_v0 returns LEXLS_ERR_UNSUPPORTED;
 *   host path (regularization_type 7, cycling handling of a regularized run, LEXLS_LSI_RESIDENT=0, shapes without a resident kernel) and the
 *     one-by-one path of deactivate_first_wrong_sign: instance b is built with row b — host factors only.
 * lexls_lsi_batch_get_lambda after a regularized run stays LEXLS_ERR_UNSUPPORTED.
 * Errors of this call: LEXLS_ERR_INVALID for a null handle; LEXLS_ERR_UNSUPPORTED for in_device_memory == 1 on a batch whose regularized runs
 * cannot be resident at all (no register-resident kernel for its shape) — the rule of lexls_lsi_batch_run_device: no detour over the host.
 * Errors of a run while the setting holds, each before any work and with every output left alone: LEXLS_ERR_INVALID when h_reg_factors is not
 * NULL; LEXLS_ERR_UNSUPPORTED when device factors are set and the regularized run would not be resident (regularization_type 7, cycling handling,
 * LEXLS_LSI_RESIDENT=0 — with host factors the same run proceeds on the host path); LEXLS_ERR_UNSUPPORTED when device factors are set and
 * lexls_lsi_batch_run is given h_v0. */
int lexls_lsi_batch_set_instance_regularization(lexls_lsi_batch_t b, const double *factors, int in_device_memory);
/* Instance mask of the device entries: "not this instance, this run".  d_mask holds `batch` bytes in the memory of the batch's device; a byte of 0
 * skips the instance for that run, any other value solves it.  The pointer is kept — no copy is made, on the host or on the device, and no run
 * reads the mask on the host — alive until the setting is cleared or the batch destroyed.  The mask is read per run: on the device, at the start
 * of every run and in the run's stream (the rule of lexls_lsi_batch_set_instance_regularization with in_device_memory = 1), so the caller may
 * rewrite the bytes in place between two runs, and a captured run reads them again at every replay.  d_mask == NULL clears the setting: the batch
 * is then what it was before the call.
 * A skipped instance is not touched.  None of its input data is interpreted: it gets no input checks and cannot raise a fault word, and NaNs in
 * its data, x0 or v0 reach no arithmetic whose result is stored anywhere.  Its caller-owned rows are untouched: d_x, d_info6, d_active, d_v,
 * d_lambda and d_cycling_counts keep the bits they had before the run.  What the library owns describes the run, a skipped instance as an empty
 * entry: working-set log count 0 and rows zero, lexls_lsi_batch_get_lambda rows zero, lexls_lsi_batch_get_cycling_counters 0.
 * A solved instance gets the bits it gets without a mask, every output row, on the persistent launch and on the lock-step stages; an input error
 * in a solved instance is reported as always (LEXLS_ERR_INVALID from the synchronous entries, d_status from the enqueued one) and names it.
 * A mask whose bytes are all 0 is a valid run that solves nothing: LEXLS_OK, a good status word, every caller-owned output untouched.
 * Served by exactly the device entries — lexls_lsi_batch_run_device, lexls_lsi_batch_run_device_ex, lexls_lsi_batch_enqueue_device — for every run
 * they serve (a batch that LEXLS_LSI_GROUPS splits: the synchronous two; the group whose first instance is lo reads the mask from byte lo).
 * lexls_lsi_batch_run is refused while the mask is set: LEXLS_ERR_UNSUPPORTED before any work, its outputs left alone — its phase 1 builds host
 * objects from host data and cannot read a device mask (no detour, as for device factors).  The one-shot lexls_lsi_batch_solve* calls make their
 * own batch object and are not concerned.  How it works: lsi_phase1_setup_kernel reads the instance's byte and leaves a skipped instance stopped
 * (not alive, the equality solver's skip byte set), so every later kernel passes over it as over a finished one; the result scatter kernels do
 * not store its rows.  Errors of this call: LEXLS_ERR_INVALID for a null handle or between lexls_lsi_batch_enqueue_device and its finish. */
int lexls_lsi_batch_set_instance_mask(lexls_lsi_batch_t b, const uint8_t *d_mask);
/* Factorization budgets per instance of the device entries: max_number_of_factorizations, the one run parameter left that was one host value for
 * the whole batch.  d_limits holds `batch` int32 in the memory of the batch's device.  The pointer is kept — no copy is made on the host and no
 * run reads the limits on the host — alive until the setting is cleared or the batch destroyed.  The limits are read per run: on the device, in
 * stream order, at the start of every lexls_lsi_batch_run_device / _run_device_ex / _enqueue_device run and of every replay of a captured one, so
 * the caller may rewrite them in place between two runs and between two replays.  d_limits == NULL clears the setting: the batch is then what it
 * was before the call.
 * An entry L >= 1: the instance runs exactly as one LexLSI object with max_number_of_factorizations = min(L, the run's parameter) — the test is
 * the reference's nFactorizations >= max (lexlsi.h:238), the status MAX_NUMBER_OF_FACTORIZATIONS_EXCEEDED where it ends the run, and x, v, the
 * working set, the info6 counters, the cycling counter, the working-set log and the multipliers are that object's, bit for bit.  An instance that
 * ends on its limit continues in the next run from its own active / x / v (the reference's anytime behaviour).  An entry L <= 0: the instance
 * has no budget of its own and takes the run's parameter.  The run's parameter stays the upper bound for everyone (it is the loop bound of the
 * persistent launch; the host knows nothing of the array).
 * The value that counts for a run is the one present when the run starts in stream order: lsi_phase1_setup_kernel, the first kernel that
 * touches the instance, copies it into the instance's resident state (a vector load of every lane), and every later kernel of the run — the
 * resident iterations' stop test, on the persistent launch and on the lock-step stages — reads that copy.  A caller kernel that rewrites the array
 * behind the enqueue in the same stream cannot change a run in flight.  The entry of an instance that an instance mask skips is not read.
 * PROBLEM_SOLVED_CYCLING_HANDLING is still tested before the limit.  With the setting off no kernel loads anything new.
 * Served by exactly the device entries, for every run they serve and with every option of theirs (deactivate_first_wrong_sign, regularized
 * runs, d_v0, d_lambda, d_cycling_counts, the working-set log, an instance mask; a batch that LEXLS_LSI_GROUPS splits: the group whose first
 * instance is lo reads the limits from word lo); lexls_lsi_batch_get_lambda, _stats, _last_kernel and _get_cycling_counters answer afterwards as
 * after any device run.  While the setting is on lexls_lsi_batch_run returns LEXLS_ERR_UNSUPPORTED before any work, its outputs left alone: its
 * phase 1 is host work and reads no device memory (the mask's rule); runs that would not be resident are refused by the device entries as always.
 * Errors of this call: LEXLS_ERR_INVALID for a null handle or between lexls_lsi_batch_enqueue_device and its finish. */
int lexls_lsi_batch_set_instance_max_factorizations(lexls_lsi_batch_t b, const int32_t *d_limits);
/* Objective row counts per instance of the device entries: the structure, the last quantity that was one value for the whole batch.  d_dims holds
 * batch x nObj uint32 in the memory of the batch's device, instance-major.  The pointer is kept — no copy is made on the host and no run reads the
 * counts on the host — alive until the setting is cleared or the batch destroyed.  The counts are read per run: on the device, in stream order, at
 * the start of every lexls_lsi_batch_run_device / _run_device_ex / _enqueue_device run and of every replay of a captured one, so the caller may
 * rewrite them in place between two runs and between two replays.  d_dims == NULL clears the setting: the batch is then what it was before the
 * call.
 * The dims of lexls_lsi_batch_create become capacities: instance i is the LexLSI problem whose objective k consists of the FIRST
 * d_dims[i * nObj + k] rows of its objective-k block.  Every layout stays the capacity layout: in d_data the leading dimension of a block is
 * still dims[k]; d_var_index holds the instance's indices in the first d_dims[i * nObj] entries of its row of dims[0] (a simple-bounds objective
 * 0); in d_active_guess, d_v0, d_active, d_v and d_lambda objective k starts at the capacity offset dims[0] + .. + dims[k-1]; d_x, d_info6 and
 * d_cycling_counts are per instance as always.
 * Rows at and beyond an instance's count are absent.  None of their data, bounds, guess, v0 or variable indices is interpreted: a NaN, lb > ub
 * or a bad index there raises no fault word and reaches no stored result.
 * Result: for every solved instance x, info6, the cycling counter and the working-set log are what ONE LexLSI object built with the instance's
 * own dims on the present rows only produces, and so are the present rows of active, v and lambda — bit for bit, on the persistent launch and
 * on the lock-step stages.  The absent rows of d_active, d_v and d_lambda are written as 0; the absent rows of lexls_lsi_batch_get_lambda are 0
 * as well; the working-set log never names an absent row.
 * A count of 0 is an empty objective and is served: the reference solves a problem with an objective of no rows (its level of the equality
 * problems is empty in every iteration), and the instance gets that object's bits.
 * An entry above its capacity is an input fault, code 5 ("objective row count above the batch's capacity"), reported like the codes 1 - 4:
 * LEXLS_ERR_INVALID from the synchronous entries with lexls_last_error() naming the instance, d_status = instance * 8 + 5 from the enqueued one;
 * nothing is solved and every output is left as it was.  It is the only check made of such an instance (its rows are not known).
 * The counts that hold for a run are those present when the run starts in stream order: lsi_phase1_setup_kernel reads them right after the mask
 * byte (a vector load), checks them and copies them into the instance's resident state, and every later kernel of the run — the resident
 * iterations' ratio test, state update and working-set lists — reads that copy.  A caller kernel that rewrites the array behind the enqueue in the
 * same stream cannot change a run in flight.  The counts of an instance that an instance mask skips are not read.  The batch is dispatched by its
 * capacities: lexls_lsi_batch_last_kernel names what a run without the setting names.  With the setting off no kernel loads anything new.
 * Served by exactly the device entries, for every run they serve and with every option of theirs (deactivate_first_wrong_sign, cycling handling
 * of an unregularized run, regularized runs with shared, host or device factors, d_x0 / d_v0, d_lambda, d_cycling_counts, the working-set log, an
 * instance mask, per-instance budgets, LEXLS_LSI_NO_FUSED=1; a batch that LEXLS_LSI_GROUPS splits: the group whose first instance is lo reads from
 * row lo).  While the setting is on lexls_lsi_batch_run returns LEXLS_ERR_UNSUPPORTED before any work, its outputs left alone: its phase 1 builds
 * host objects and reads no device memory (the mask's rule).
 * Errors of this call: LEXLS_ERR_INVALID for a null handle or between lexls_lsi_batch_enqueue_device and its finish. */
int lexls_lsi_batch_set_instance_obj_dims(lexls_lsi_batch_t b, const uint32_t *d_dims);
/* How a run executes: phase 1 of every instance on the host; from then on the instance's active-set iterations are resident on the
 * device (LEXLS_LSI_RESIDENT=0: host logic, lock-step stages).  Where the batch's shape has a persistent instantiation (the register-resident l-QR shapes:
 * nVar + 1 <= 41 with levels of up to 12 rows, nVar + 1 <= 64 with levels of up to 16 — except 42..48 columns), everything behind the first resident
 * stage is ONE launch: per instance l-QR -> step -> removal search behind an unblocked step -> working-set change, until the instance stops
 * (LEXLS_LSI_NO_FUSED=1, read per run: three launches per lock-step stage instead; same results bit for bit).
 * A regularized run (regularization_type 1..6, 8, 9) takes the same route: its regularization — type, variable factor, CG iteration bound and one
 * factor per LexLSE level (objective k + 1's for level k when objective 0 holds simple bounds, which become fixed variables and are not
 * regularized) — is put on the device once per run, in every group's stream, and the l-QR of an iteration is the regularized instantiation of the
 * register-resident kernel, inside the persistent launch or as the stage's l-QR launch.  Such an iteration refactorizes every level (the
 * null-space basis the damping reads accumulates over the levels: no prefix reuse).  Where the regularization routines' LDS does not fit the
 * persistent launch's 64 KB the stages are taken, where it does not fit a workgroup at all the host path.  Host path as before, whatever the
 * type: regularization_type 7, cycling handling of a regularized run, shapes without a register-resident kernel.
 * cycling_handling_enabled (cycling.h:32-65) is part of the resident iteration of an unregularized run (regularization_type 0): the handler of
 * every instance — its last working-set change, the relaxations it has done — travels with the instance when it leaves the host; an ADD of the
 * (objective, constraint, type) that was just REMOVEd moves that bound by cycling_relax_step in the instance's resident constraint data, where the
 * next equality problems, the step and v read it; after cycling_max_counter relaxations the instance ends PROBLEM_SOLVED_CYCLING_HANDLING (tested
 * before the factorization limit, as lexlsi.h does).  Persistent launch and stages alike.  The caller's h_data is never written, and every run
 * uploads it anew: nothing of a run's relaxations reaches the next one.  A REGULARIZED run with cycling handling keeps the host path (its
 * instances relax their host copies of the bounds and the equality problems are assembled from those), as do LEXLS_LSI_RESIDENT=0, shapes
 * without a register-resident kernel and data that is not resident (LEXLS_LSI_HOST_STAGING).
 * deactivate_first_wrong_sign (lexlsi.h:1063-1105) is a removal RULE, not another path: a run that would be resident without it is resident with
 * it — the removal search collects the wrong-sign set (lexls_lse_sensitivity_collect) and the iteration removes its member that entered the
 * working set first (an activation stamp per constraint carries the order of the reference's WS list).  Where such a run would not be resident
 * (LEXLS_LSI_RESIDENT=0, cycling handling of a regularized run, type 7, no register-resident kernel, data not resident) its instances go through the single-problem
 * driver one after the other.
 * Phase 1 as device work: lexls_lsi_batch_run_device always, lexls_lsi_batch_run when LEXLS_LSI_DEVICE_PHASE1=1 is in the environment (read per
 * run; off by default) and the run is resident and has no h_v0 — otherwise the switch changes nothing.  No host LexLSI objects are built: one
 * kernel does the input checks and equality activations of LexLSI::setData, api_activate over the guess (the working-set lists and activation
 * stamps in the reference's order), A x0 and v0, and writes the first equality problem into the equality solver's in slab; the stage of every
 * resident iteration follows (l-QR + speculative removal search), then iteration 0 as the resident iteration itself (without x0: on x = the
 * solution of the first problem, with dx = 0).  Same results bit for bit, the same kernels named by lexls_lsi_batch_last_kernel, phase 1's stage
 * counted by lexls_lsi_batch_stats like any other.  The host path's printf warnings are not reproduced; the input faults above are errors.
 * lexls_lsi_batch_stats:
 * of the last lexls_lsi_batch_run: {factorize+solve stages, sensitivity stages, stages whose iteration step ran on the device, groups}.
 * The step of an iteration (A*dx, ratio test, update of x / v / A*x: lexlsi.h:987-1029, :1234-1240) runs on the device
 * next to the equality solve when the batch is created with LEXLS_LSI_DEVICE_STEP=1 in the environment; off by default. */
int lexls_lsi_batch_stats(lexls_lsi_batch_t b, int32_t *h_stats4);
int lexls_lsi_batch_destroy(lexls_lsi_batch_t b);
/* LexLSI::getLambda (lexlsi.h:552-605) of every instance of the LAST lexls_lsi_batch_run on this batch: h_lambda receives batch x total x nObj
 * doubles — per instance the `lambda` of lexls_lsi_debug (total x nObj, column-major, objectives stacked, user's constraint order), instances back
 * to back.  Row of an active constraint = its multipliers in the equality problem of the instance's final working set (placed through
 * getActiveCtrIndex, :592-604); inactive constraints 0; column 0 zero when objective 0 holds simple bounds (nObjOffset), the active simple bounds'
 * rows carrying the fixed-variable multipliers.  Computed on request only, on the device in the batch's streams: the final equality problems are
 * formed from the working sets the run kept (rows gathered from the resident constraint data), factorized with the factor kept on a bit-exact
 * kernel — the same factor for instances that ended PROBLEM_SOLVED and for those the reference re-forms and refactorizes first (:568-571) —,
 * every objective's multipliers taken at once (lexls_lse_multipliers), scattered into user order, copied back.  Bit-identical to
 * lexls_lsi_solve_debug's `lambda` on each instance, every run path included (persistent launch, lock-step stages, LEXLS_LSI_RESIDENT=0, warm
 * starts, v0, factorization limits, deactivate_first_wrong_sign), factorized with the run's tol_linear_dependence.
 * Cost to runs that never ask: none, except for a deactivate_first_wrong_sign run that is NOT resident — its instances go one by one through the
 * single-problem driver, which never uses the batch's handles, so the constraint data is copied to the device once per run (what get_lambda
 * gathers from later); a resident run with that rule has the data there already, like any other.
 * Errors: LEXLS_ERR_INVALID before any run (or after a failed one); LEXLS_ERR_UNSUPPORTED after ANY run with cycling_handling_enabled (it may have
 * relaxed bounds — in the instances' host copies on the host path, in the resident constraint data of a resident run — and the final equality
 * problems are not re-formed from relaxed data after the run), after a regularized run (regularization_type != 0), or when the batch's constraint data is not resident
 * (LEXLS_LSI_HOST_STAGING, data beyond 2^31 doubles per instance) or holds more than 65535 constraints per instance.  A later run replaces the multipliers of the previous one. */
int lexls_lsi_batch_get_lambda(lexls_lsi_batch_t b, double *h_lambda);
/* Gradients of the LAST completed run's solutions with respect to the bounds, the matrices A HELD FIXED.  At an instance that ended
 * PROBLEM_SOLVED, x is the basic solution of the equality problem of its final working set W: the right-hand sides are the active bounds (lb or
 * ub by activation type), the fixed values the active simple bounds.  While W does not change x is exactly affine in the bounds, so with
 * g = dloss/dx these calls return dloss/dlb and dloss/dub: the final equality problems are formed and factorized with the factor kept as for
 * lexls_lsi_batch_get_lambda (once per run: whichever of the two is called first pays for it, every later call of either reuses the factor),
 * lexls_lse_solve_adjoint_device gives M^T g and N^T g, and lsi_adjoint_scatter_multi_kernel (with one cotangent) takes them from LOD-row /
 * fixed-slot order back to the user's constraint order.  These calls give NO derivatives with respect to A: lexls_lsi_batch_solve_adjoint_matrix, below, does.
 * Layouts: g is batch x nVar, dloss/dx in the user's variable order; grad_lb and grad_ub are batch x sum(dims) each, in the constraint order of
 * h_active / h_v (objective by objective).  Either output may be NULL (not wanted).  lexls_lsi_batch_solve_adjoint takes and fills host arrays;
 * lexls_lsi_batch_solve_adjoint_device takes memory of the batch's device, and no gradient, g or factor passes through host memory.  Both are
 * host-synchronous like lexls_lsi_batch_run_device: the inputs have to be complete at the call, the outputs are complete at the return.
 * Solved instances (status PROBLEM_SOLVED), per constraint of the final working set: CTR_ACTIVE_LB — the value goes to grad_lb, grad_ub is 0;
 * CTR_ACTIVE_UB — the value goes to grad_ub, grad_lb is 0; CTR_ACTIVE_EQ — the value goes to grad_ub, the bound the final equality problem
 * reads, and grad_lb is 0 (with lb = ub = c the caller's dloss/dc is the sum of the two either way).  Active simple bounds of objective 0 take
 * grad_fixed of their slot, by the same rule.  Every constraint that is not in the working set is exactly 0, and so are the rows that are absent
 * under lexls_lsi_batch_set_instance_obj_dims.
 * Status rule: an instance with ANY OTHER status (stopped by a factorization budget, for instance) gets zeros in all its rows of both outputs —
 * its x is an intermediate iterate, not the solution of its working set's equality problem.  The status is the one the run left behind (its host
 * object's, or the resident slab's), never read from an array of the caller.
 * Mask rule: an instance that the instance mask (lexls_lsi_batch_set_instance_mask) skips keeps the bits of its rows in both outputs, like every
 * other output under the mask.
 * The gradient is that of the piece of the piecewise-affine map the solve ended on: where a constraint sits at its bound without being in the
 * working set it is one-sided.  Tolerance contract, as for lexls_lse_solve_adjoint; the same bits from run to run and from the host and the
 * device form.  x, active, v and the multipliers of the run are not touched.
 * Errors, each returned before any device work and with every output left alone: LEXLS_ERR_INVALID for a null handle, a null g, or both
 * outputs null; LEXLS_ERR_INVALID when the batch has no completed run, or a lexls_lsi_batch_enqueue_device run is waiting for
 * lexls_lsi_batch_finish; LEXLS_ERR_UNSUPPORTED after exactly the runs for which lexls_lsi_batch_get_lambda answers LEXLS_ERR_UNSUPPORTED (cycling
 * handling, a regularized run, more than 65535 constraints, constraint data not resident), with that call's reason in lexls_last_error(). */
int lexls_lsi_batch_solve_adjoint(lexls_lsi_batch_t b, const double *h_g, double *h_grad_lb, double *h_grad_ub);
int lexls_lsi_batch_solve_adjoint_device(lexls_lsi_batch_t b, const double *d_g, double *d_grad_lb, double *d_grad_ub);
/* on != 0: from the NEXT run on, the two calls above also answer after a regularized run that was resident on the device, of regularization
 * type 1, 3, 4, 5, 8 or 9 with variable_regularization_factor == 0: the final equality problems are then factorized WITH the run's regularization
 * (type, and the shared or per-instance factors, host or device rows, whichever the run used: they are on the groups' handles since the run),
 * once per run as before, and the gradient is that of the damped solve, the factors held fixed as the matrices are.  Per-instance factors in
 * device memory are read again at that factorization: rows rewritten in place between the run and the first adjoint call give the adjoint of the
 * rewritten factors, and no error is raised.  0 (the default, so that a caller who takes LEXLS_ERR_UNSUPPORTED after a regularized run as the
 * sign to differentiate some other way keeps getting it): every regularized run is refused.  Types 2, 6, 7, a variable factor, cycling handling,
 * a run that was not resident and more than 65535 constraints stay LEXLS_ERR_UNSUPPORTED, and so do lexls_lsi_batch_get_lambda and
 * lexls_lsi_batch_solve_adjoint_matrix* after every regularized run, and lexls_lsi_batch_solve_adjoint_multi* unless
 * lexls_lsi_batch_set_adjoint_regularized_multi (below) was on for the run.
 * Errors: LEXLS_ERR_INVALID for a null handle, and between lexls_lsi_batch_enqueue_device and lexls_lsi_batch_finish. */
int lexls_lsi_batch_set_adjoint_regularized(lexls_lsi_batch_t b, int on);
/* lexls_lsi_batch_solve_adjoint(_device) for ncot cotangents per instance in one pass: lexls_lse_solve_adjoint_multi_device on the final factor
 * (shared with lexls_lsi_batch_get_lambda and lexls_lsi_batch_solve_adjoint in every call order: nothing is factorized twice), then
 * lsi_adjoint_scatter_multi_kernel.  Layouts: G is batch x ncot x nVar; grad_lb and grad_ub are batch x ncot x sum(dims), row c of instance b
 * what lexls_lsi_batch_solve_adjoint returns for g = G[b][c] (tolerance contract; the exact zeros at the same entries).  Either output may be
 * NULL.  The status rule (exact zeros unless PROBLEM_SOLVED), the mask rule (a skipped instance keeps the bits of all its ncot rows) and the
 * absent-row rule are those of lexls_lsi_batch_solve_adjoint, and so are the errors, with LEXLS_ERR_INVALID for ncot == 0 added: each is
 * returned before any device work and with every output left alone.  The independence contract of lexls_lse_solve_adjoint_multi holds. */
int lexls_lsi_batch_solve_adjoint_multi(lexls_lsi_batch_t b, const double *h_G, uint32_t ncot, double *h_grad_lb, double *h_grad_ub);
int lexls_lsi_batch_solve_adjoint_multi_device(lexls_lsi_batch_t b, const double *d_G, uint32_t ncot, double *d_grad_lb, double *d_grad_ub);
/* on != 0: from the NEXT run on, the two calls above also answer after a regularized run, under the conditions
 * lexls_lsi_batch_set_adjoint_regularized states for the single call (a resident run of type 1, 3, 4, 5, 8 or 9, a zero variable factor, no
 * cycling handling, at most 65535 constraints), through lexls_lse_set_adjoint_regularized_multi on the groups' handles.  The final factor is
 * the damped one, factorized once per run and shared with lexls_lsi_batch_solve_adjoint when both switches are on.  Independent of that
 * switch.  0 (the default): the refusal of a regularized run is the one of lexls_lsi_batch_get_lambda, with this switch named.
 * Errors: LEXLS_ERR_INVALID for a null handle, and between lexls_lsi_batch_enqueue_device and lexls_lsi_batch_finish. */
int lexls_lsi_batch_set_adjoint_regularized_multi(lexls_lsi_batch_t b, int on);
/* Gradients of the LAST completed run's solutions with respect to ALL constraint data — the matrices A and the bounds — in the caller's layout.
 * At an instance that ended PROBLEM_SOLVED, x is the basic solution of the equality problem of its final working set W; while W holds, x as a
 * function of the active rows' A and bounds is the LexLSE solve map of that final problem, so the gradient is lexls_lse_solve_adjoint_matrix's,
 * applied to the final problem and carried back to the user's constraint order: the final factor is the one lexls_lsi_batch_get_lambda and
 * lexls_lsi_batch_solve_adjoint keep (shared in every call order: nothing is factorized twice), its x is solved for once per run, the matrix chain
 * of the equality solver runs on it (N^T g comes out of the chain's own solve_adjoint launch), lsi_adjoint_matrix_scatter_kernel writes the result.
 * Layouts: g is batch x nVar, dloss/dx in the user's variable order.  grad_data is batch x the per-instance data length, exactly the layout
 * lexls_lsi_batch_run_device reads: per objective a column-major dim x w block, w = nVar + 2 for a general objective ([A | lb | ub]), w = 2 for
 * simple bounds ([lb | ub]).  differentiable is one byte per instance (NULL: not wanted); grad_data may not be NULL.
 * Per constraint of the final working set of a differentiable instance: an active general row gets its row of - y x^T - lambda u^T in the A
 * columns and its entry of y = M^T g in the lb column (CTR_ACTIVE_LB) or the ub column (CTR_ACTIVE_UB, CTR_ACTIVE_EQ: the bound the final problem
 * reads, as in lexls_lsi_batch_solve_adjoint), the other bound column 0; an active simple bound of objective 0 gets its slot of N^T g by the same
 * type rule.  Every row that is not in W, and every row absent under lexls_lsi_batch_set_instance_obj_dims, is exact zeros.  As for the bounds,
 * this is the gradient of the piece of the map the solve ended on.
 * Flag rule: differentiable = 1 when the instance's status is PROBLEM_SOLVED and its final equality problem is rank-stable by the rule of
 * lexls_lse_solve_adjoint_matrix, evaluated by that call's kernel on the final problem's levels, ranks and fixed count; an instance with an empty
 * working set is differentiable (and all zeros).  Otherwise the flag is 0 and the WHOLE slice of the instance is exact zeros, bound columns
 * included — the convention of grad_lod.  lexls_lsi_batch_solve_adjoint still gives a solved instance whose final problem is not rank-stable its
 * bound gradients (they exist for A held fixed).
 * Mask rule: an instance that the instance mask skips keeps the bits of its slice and of its flag.
 * lexls_lsi_batch_solve_adjoint_matrix takes and fills host arrays (staged in buffers of the groups); the _device form takes memory of the
 * batch's device, and no gradient, g or factor passes through host memory.  Both are host-synchronous like lexls_lsi_batch_solve_adjoint(_device).
 * Tolerance contract; no atomics, the same bits from run to run and from the host and the device form.  What lexls_lsi_batch_get_lambda,
 * lexls_lsi_batch_solve_adjoint(_multi) and the run's x / active / v answer is unchanged, bit for bit, before and after these calls.
 * Errors, each returned before any device work and with every output left alone: LEXLS_ERR_INVALID for a null handle, a null g or a null
 * grad_data; otherwise exactly those of lexls_lsi_batch_solve_adjoint (no completed run, an enqueue_device run waiting for finish; cycling
 * handling, a regularized run, more than 65535 constraints, constraint data not resident: LEXLS_ERR_UNSUPPORTED). */
int lexls_lsi_batch_solve_adjoint_matrix(lexls_lsi_batch_t b, const double *h_g, double *h_grad_data, uint8_t *h_differentiable);
int lexls_lsi_batch_solve_adjoint_matrix_device(lexls_lsi_batch_t b, const double *d_g, double *d_grad_data, uint8_t *d_differentiable);
/* FORWARD-MODE tangents of a batch's solutions with respect to its constraint data: how x of the last run moves along ntan directions per
 * instance, while the working set holds — lexls_lse_solve_tangent on the final equality problem of every instance, the transpose of
 * lexls_lsi_batch_solve_adjoint_matrix.
 * Layouts: ddata is ntan x batch x per-instance data doubles, direction c of instance b in exactly the layout lexls_lsi_batch_run_device reads
 * (per objective a column-major dim x w block, [dA | dlb | dub], or [dlb | dub] for simple bounds); dx is ntan x batch x nVar; differentiable
 * (may be NULL) is one byte per instance, the flags lexls_lsi_batch_solve_adjoint_matrix writes.
 * An active general row contributes its dA row and its dlb (CTR_ACTIVE_LB) or dub (CTR_ACTIVE_UB, CTR_ACTIVE_EQ: the bound the final problem
 * reads); an active simple bound contributes its entry of dlb / dub by the same rule as the tangent of that fixed value.  Rows outside the
 * working set, and rows absent under lexls_lsi_batch_set_instance_obj_dims, are never read: a NaN there changes nothing.
 * An instance that did not end PROBLEM_SOLVED, or whose final problem is not rank-stable, gets flag 0 and exact zeros in its rows of dx; an
 * empty working set is differentiable with dx = 0; with an instance mask set a skipped instance keeps the bits of its rows and of its flag.
 * The final factor and its x are shared with lexls_lsi_batch_get_lambda and every adjoint call, in any call order
 * (lexls_lsi_batch_final_factorizations still counts one formation per run and group).  Both forms are host-synchronous like
 * lexls_lsi_batch_solve_adjoint_matrix(_device); the _device form takes memory of the batch's device and nothing passes through host memory.
 * Tolerance contract; no atomics, the same bits from run to run and from the host and the device form.
 * Errors, each returned before any device work and with every output left alone: LEXLS_ERR_INVALID for a null handle, a null ddata, a null dx
 * or ntan == 0; otherwise exactly those of lexls_lsi_batch_solve_adjoint_matrix. */
int lexls_lsi_batch_solve_tangent(lexls_lsi_batch_t b, const double *h_ddata, uint32_t ntan, double *h_dx, uint8_t *h_differentiable);
int lexls_lsi_batch_solve_tangent_device(lexls_lsi_batch_t b, const double *d_ddata, uint32_t ntan, double *d_dx, uint8_t *d_differentiable);
/* NEW BOUNDS on the final working set: the finite-step counterpart of the gradient calls.  While an instance's working set W holds, its x is an
 * affine map of the bounds; these calls apply that map to nrhs other bound sets per instance and say how far each answer leaves the region where
 * W can be valid: lsi_bounds_gather_kernel turns the bound sets into right-hand sides of the final equality problems, lexls_lse_solve_rhs_device
 * solves them on the kept final factor (nothing is factorized again), lsi_bounds_check_kernel writes x and measures every answer against ALL rows
 * of the instance in the constraint data that stayed resident from the run.
 * Layouts: lb and ub are nrhs x batch x sum(dims) each, in the user's constraint order (the row order of grad_lb / grad_ub of
 * lexls_lsi_batch_solve_adjoint); x is nrhs x batch x nVar; violation is nrhs x batch (NULL: not wanted); valid is batch bytes (NULL: not wanted).
 * Meaning: x[c, i] solves the final equality problem of instance i's last run — its final working set as lexls_lsi_batch_get_lambda forms it —
 * with the bounds replaced by bound set c: an active general row of type CTR_ACTIVE_LB takes lb[c, i, row], CTR_ACTIVE_UB and CTR_ACTIVE_EQ take
 * ub[c, i, row] (the bound the final problem reads, as in lexls_lsi_batch_solve_adjoint); an active simple bound fixes its variable at the bound
 * chosen by the same rule.  Rows outside the working set contribute nothing to x.  With the run's own bounds x is the run's x within the
 * tolerance contract of lexls_lse_solve_rhs.
 * valid[i] = 1 when instance i ended PROBLEM_SOLVED, else 0 — and then all its rows of x and of violation are exact zeros (the convention of
 * `differentiable`, without the rank-stability condition: lexls_lse_solve_rhs serves rank-deficient factors, and so does this call).  An empty
 * working set gives x = 0, and its violation is measured against that x.
 * violation[c, i] is the largest amount by which x[c, i] breaks a bound of bound set c, over all sum(dims) rows of all objectives, in or out of
 * W: for a general row max(lb - a.x, a.x - ub, 0), for a simple bound the same with x[var] for a.x, and for every row, active ones included,
 * max(lb - ub, 0).  a.x is one ordered fma chain over the variables 0 .. nVar - 1.  Rows absent under lexls_lsi_batch_set_instance_obj_dims are
 * never read (a NaN in lb / ub there reaches nothing).
 * WHAT THE VIOLATION DOES NOT SAY: violation <= tol is NECESSARY for the working set to remain the LexLSI answer under the new bounds, NOT
 * SUFFICIENT.  The signs of the multipliers under the new bounds are not re-examined: an answer with violation 0 may still be one that the
 * active-set method would leave by dropping a constraint.  A caller who needs certainty warm-starts lexls_lsi_batch_run_device from the working
 * set.  Rows of lower priority that the lexicographic optimum itself leaves unmet count as well: the figure to compare with is the violation of
 * the run's own bounds, not 0.  Thresholding is the caller's: the library fixes no tolerance.
 * Mask rule: an instance that the instance mask skips keeps the bits of its rows of all three outputs (the host form copies the caller's arrays
 * in first).  The final factor is shared with lexls_lsi_batch_get_lambda and every gradient call, in any call order
 * (lexls_lsi_batch_final_factorizations still counts one formation per run and group); what those calls answer is unchanged by this one.
 * Both forms are host-synchronous like lexls_lsi_batch_solve_tangent(_device); the _device form takes memory of the batch's device and nothing
 * passes through host memory.
 * Independence contract, inherited from lexls_lse_solve_rhs and kept by both kernels: for nrhs >= 2, x and violation of a bound set do not depend
 * on nrhs, on its position or on its company, bit for bit (one lane per bound set, no cross-lane sums, no atomics); the same bits come back from
 * run to run and from the host and the device form.  Between nrhs == 1 and nrhs >= 2 the contract is the tolerance one.
 * Errors, each returned before any device work and with every output left alone: LEXLS_ERR_INVALID for a null handle, a null lb, ub or x,
 * nrhs == 0 or nrhs > 65535, when the batch has no completed run, or when a lexls_lsi_batch_enqueue_device run is waiting for
 * lexls_lsi_batch_finish; LEXLS_ERR_UNSUPPORTED after exactly the runs for which lexls_lsi_batch_solve_tangent answers it (cycling handling, a
 * regularized run, more than 65535 constraints, constraint data not resident).
 * Kernel variant (lexls_lsi_batch_last_consumer_kernel): "lsi_bounds_check<lds>" — the x vectors of a wavefront's 64 bound sets transposed in
 * LDS — or "lsi_bounds_check<hbm>" — each lane reads its own where the solver left it —, decided from nVar alone (lds up to nVar 46).
 * Cost: a call costs about the same for 1 as for 64 bound sets. */
int lexls_lsi_batch_solve_bounds(lexls_lsi_batch_t b, const double *h_lb, const double *h_ub, uint32_t nrhs, double *h_x, double *h_violation, uint8_t *h_valid);
int lexls_lsi_batch_solve_bounds_device(lexls_lsi_batch_t b, const double *d_lb, const double *d_ub, uint32_t nrhs, double *d_x, double *d_violation, uint8_t *d_valid);
/* PER-OBJECTIVE COST of new bounds: lexls_lsi_batch_solve_bounds(_device) with one more output, the figure that ranks the nrhs candidates.
 * Everything is as there, except: cost must be non-NULL and x may be NULL (not wanted).  cost is nrhs x batch x nObj:
 *     cost[c, i, k] = sum over the rows r of objective k, in the user's row order, of d_r^2,   d_r = max(lb - a.x, a.x - ub, 0)
 * with lb, ub of bound set c and a.x the very fma chain violation uses (a simple bound: x[var]); the sum is one ordered fma chain by the lane that
 * owns bound set c.  This is the squared norm of LexLSI's v for objective k at x[c, i], measured against bound set c for ALL rows, in or out of
 * the working set: it depends on x and the bounds alone.  (violation also counts max(lb - ub, 0) of a row; cost does not: violation^2 >= every
 * d_r^2.)  Rows absent under lexls_lsi_batch_set_instance_obj_dims are never read and contribute nothing; instances with valid == 0 get exact
 * zeros; a masked instance keeps its bits of cost as of the other outputs (the host form copies the caller's arrays in first).  The independence
 * contract, the errors (a null cost in the place of a null x) and the LEXLS_ERR_UNSUPPORTED runs are those of lexls_lsi_batch_solve_bounds; the
 * final factor is shared as before.  A call of lexls_lsi_batch_solve_bounds(_device) launches exactly what it launched before these existed.
 * Kernel variant (lexls_lsi_batch_last_consumer_kernel): "lsi_bounds_cost<lds>" or "lsi_bounds_cost<hbm>", the same rule of nVar.
 * Cost: DESIGN.md 5.15. */
int lexls_lsi_batch_solve_bounds_cost(lexls_lsi_batch_t b, const double *h_lb, const double *h_ub, uint32_t nrhs, double *h_x, double *h_violation, double *h_cost,
                                      uint8_t *h_valid);
int lexls_lsi_batch_solve_bounds_cost_device(lexls_lsi_batch_t b, const double *d_lb, const double *d_ub, uint32_t nrhs, double *d_x, double *d_violation, double *d_cost,
                                             uint8_t *d_valid);
/* The kernel variant that served the LAST lexls_lsi_batch_solve_bounds(_device) or _solve_bounds_cost(_device) call on this batch (a string the
 * library owns); "" before the first such call or for a null handle. */
const char *lexls_lsi_batch_last_consumer_kernel(lexls_lsi_batch_t b);
/* How often, since the batch was created, the final equality problems of a group were formed and factorized: the stage lexls_lsi_batch_get_lambda,
 * lexls_lsi_batch_solve_adjoint(_multi), lexls_lsi_batch_solve_adjoint_matrix, lexls_lsi_batch_solve_tangent and lexls_lsi_batch_solve_bounds share.  It grows by the number of groups at the first of these
 * calls behind a run and not at all at the later ones, in every call order.  Host bookkeeping only.  LEXLS_ERR_INVALID for a null argument. */
int lexls_lsi_batch_final_factorizations(lexls_lsi_batch_t b, uint32_t *h_count);
/* LexLSI::getCyclingCounter() (lexlsi.h, CyclingHandler::get_counter, cycling.h) of every instance of the LAST lexls_lsi_batch_run on this batch:
 * h_counts receives `batch` values, the bounds each instance's cycling handler relaxed (the working-set log's cycling_detected entries, counted).
 * Whatever path served the run: host path, lock-step stages, persistent launch, one by one through the single-problem driver.  All zeros after a
 * run without cycling handling.  Errors: LEXLS_ERR_INVALID before the first run or after a failed one. */
int lexls_lsi_batch_get_cycling_counters(lexls_lsi_batch_t b, uint32_t *h_counts);
/* LexLSI::getWorkingSetLog() (lexlsi.h:739; the entries verifyWorkingSet makes at :1186-1230, which the MEX front end returns in its fifth output)
 * for every instance of a batch: one entry per working-set change — which constraint of which objective was added or removed, with which type,
 * at which step length or multiplier, whether the cycling handler relaxed a bound on it, and the rank of that iteration's factorization.
 * Row layout of lexls_lsi_debug::log: LEXLS_LSI_LOG_FIELDS int32 per entry, at the indices below, plus one double (alpha_or_lambda).
 *   ADD (lexlsi.h:1188-1194): the blocking constraint, its type (CTR_ACTIVE_LB / _UB), alpha_or_lambda = the step length alpha.
 *   REMOVE (lexlsi.h:1214-1222): the constraint's index in its objective, ctr_type = CTR_INACTIVE (0), alpha_or_lambda = lambda_wrong_sign, the
 *     largest wrong-sign multiplier of the removal search (lexlsi.h:1115-1139) — 0 under deactivate_first_wrong_sign (lexlsi.h:1069).
 *   cycling_detected (lexlsi.h:1252-1259): 1 on the ADD that closed a REMOVE -> ADD circle and relaxed a bound; the ADD that ends the run at
 *     cycling_max_counter (PROBLEM_SOLVED_CYCLING_HANDLING) is logged with 0, as CyclingHandler::update reports it (cycling.h:32-65).
 * lexls_lsi_batch_set_working_set_log: max_entries > 0 switches the log on for every later run of the object — lexls_lsi_batch_run,
 * lexls_lsi_batch_run_device, lexls_lsi_batch_run_device_ex — with room for max_entries entries per instance; 0 switches it off and frees the
 * buffers (the batch is then what it is without this call).  Every path a run can take is served and none is refused because the log is on:
 * the resident iterations (persistent launch, lock-step stages, phase 1 on the host or on the device) write their entries on the device where
 * the working-set change is decided; what an instance does on the host before it becomes resident (iteration 0), and everything of an instance
 * that never does (host path: LEXLS_LSI_RESIDENT=0, regularization type 7, cycling handling of a regularized run; the one-by-one path), is
 * logged by its host LexLSI object (ParametersLexLSI::log_working_set_enabled) and merged in.  Results and kernels of a run are the same with
 * the log on or off.  Errors: LEXLS_ERR_INVALID for a null handle. */
#define LEXLS_LSI_LOG_FIELDS 5
enum
{
    LEXLS_LSI_LOG_OBJ_INDEX        = 0,
    LEXLS_LSI_LOG_CTR_INDEX        = 1,
    LEXLS_LSI_LOG_CTR_TYPE         = 2,
    LEXLS_LSI_LOG_CYCLING_DETECTED = 3,
    LEXLS_LSI_LOG_RANK             = 4
};
int lexls_lsi_batch_set_working_set_log(lexls_lsi_batch_t b, uint32_t max_entries);
/* The log of the LAST run: h_log receives batch x max_entries x LEXLS_LSI_LOG_FIELDS int32, h_alpha batch x max_entries doubles, h_counts
 * `batch` values = the entries each instance produced (getWorkingSetLog().size()).  A count may exceed max_entries: the entries beyond the
 * capacity are dropped, as lexls_lsi_solve_debug drops those beyond max_log; rows at and behind min(count, max_entries) are zero.  Any pointer
 * may be NULL.  Errors: LEXLS_ERR_INVALID for a null handle, before the first run, after a failed one, and when the last run ran with the log off. */
int lexls_lsi_batch_get_working_set_log(lexls_lsi_batch_t b, int32_t *h_log, double *h_alpha, uint32_t *h_counts);
/* The same three arrays where the library keeps them, in the memory of the batch's device, for a consumer that stays there (lexls_lsi_batch_run_device_ex
 * itself is unchanged): *d_log, *d_alpha, *d_counts (any may be NULL) receive pointers the library owns, in the layouts above, valid until the next
 * lexls_lsi_batch_set_working_set_log or the destruction of the batch.  They describe the last run completely once the run call has returned — after
 * a run whose instances did not all stay resident, the merged log has been uploaded before that.  Errors: LEXLS_ERR_INVALID for a null handle or
 * while the log is off. */
int lexls_lsi_batch_working_set_log_device(lexls_lsi_batch_t b, void **d_log, void **d_alpha, void **d_counts);
/* lexls_lsi_solve plus what the MEX front end also passes (interfaces/matlab-octave/lexlsi.cpp:527-625): h_v0 = initial residuals,
 * sum(dims) doubles (set_v0 per objective) or NULL; h_reg_factors = one regularization factor per objective or NULL; h_params with
 * nparams == 9 (as lexls_lsi_solve), 12: + regularization_type, variable_regularization_factor, max_number_of_CG_iterations, or 17: + the five
 * hot-start options (the 17-slot form, described at lexls_lsi_solve). */
int lexls_lsi_solve_ex(int device, uint32_t nVar, uint32_t nObj, const uint32_t *h_dims, const int32_t *h_types, const double *h_data,
                       const uint32_t *h_var_index, const uint8_t *h_active_guess, const double *h_x0, const double *h_v0,
                       const double *h_reg_factors, const double *h_params, uint32_t nparams, double *h_x, int32_t *h_info6, uint8_t *h_active,
                       double *h_v);
/* The fifth output of the MEX front end, `[x, info, v, as, d] = lexlsi(...)` (interfaces/matlab-octave/lexlsi.cpp:739-770,
 * formDebugStructure :77-260): lexls_lsi_solve_ex with the working-set log on (ParametersLexLSI::log_working_set_enabled), followed by the
 * getter sequence of :752-762.  Every pointer of `debug` may be NULL.  total = sum(dims); rows = row capacity of the equality solver
 * (total, minus dims[0] when objective 0 holds simple bounds); nObjL = its number of levels. */
typedef struct lexls_lsi_debug
{
    double *lambda;       /* total x nObj, column-major: getLambda() lexlsi.h:552-605, objectives stacked, user's constraint order   */
    double *lexqr, *data; /* rows x (nVar+1), column-major, ld = rows: get_lexqr() :632, get_data() :637 of the last equality problem */
    double *x_star;       /* nVar: get_xStar() :519                                                                                */
    int32_t *active_ctr;  /* total x 3: (obj_index, ctr_index, ctr_type) in working-set order, getActiveCtr_order() :703            */
    int32_t *log;         /* max_log x 5: (obj_index, ctr_index, ctr_type, cycling_detected, rank) per change, getWorkingSetLog()  */
    double *log_alpha;    /* max_log: alpha_or_lambda of the entry                                                                 */
    uint32_t max_log;
    double *x_mu, *x_mu_rhs, *residual_mu; /* REGULARIZATION_TIKHONOV_1 only (:617-630): nObjL x nVar (column k contiguous) twice, rows */
    uint32_t *counts;     /* 4: rows, nObjL, number of active constraints, number of log entries (entries beyond max_log are dropped) */
} lexls_lsi_debug;
int lexls_lsi_solve_debug(int device, uint32_t nVar, uint32_t nObj, const uint32_t *h_dims, const int32_t *h_types, const double *h_data,
                          const uint32_t *h_var_index, const uint8_t *h_active_guess, const double *h_x0, const double *h_v0,
                          const double *h_reg_factors, const double *h_params, uint32_t nparams, double *h_x, int32_t *h_info6, uint8_t *h_active,
                          double *h_v, const lexls_lsi_debug *debug);
/* the same on a hierarchy file in the reference's .dat format (tools.h:261-453); h_solution receives the file's
 * `#Solution` block when present (may be NULL).  one_based: simple-bound indices in the file are 1-based. */
int lexls_lsi_solve_dat(int device, const char *path, int one_based, int use_active_guess, int use_x_guess, double *h_x, int32_t *h_info6,
                        double *h_solution);
/* The kernel that served the resident active-set iterations of the LAST lexls_lsi_batch_run on this batch (a string the library owns):
 * "lsi_fused<lqr_wave<41,12,exact>>", "lsi_fused<lqr_wave<41,12,regularized>>", ... for the persistent launch; the l-QR kernel of the last
 * lock-step stage ("lqr_wave<41,12,regularized>", "lqr_quad<3,12,factor,fixed>", ...) where the stages ran (LEXLS_LSI_NO_FUSED=1, or no
 * persistent instantiation); "host" when no instance's iterations were resident (LEXLS_LSI_RESIDENT=0, regularization_type 7, cycling handling of a
 * regularized run, every instance done in phase 1); "" before the first run.  Neither deactivate_first_wrong_sign nor cycling handling of an
 * unregularized run changes the name. */
const char *lexls_lsi_batch_last_kernel(lexls_lsi_batch_t b);

#ifdef __cplusplus
}
#endif
#endif /* LEXLS_HIP_H */
