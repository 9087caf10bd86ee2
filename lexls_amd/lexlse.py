"""Host-side mirror of the reference's equality solver for a BATCH of problems, over the C ABI.

``BatchedLexLSE`` keeps the reference's method names and call order
(LexLS::internal::LexLSE, include/lexls/lexlse.h: resize :67, setObjDim :1426, setParameters :1467,
fixVariables :1398, setCtrType :1548, setProblem :1511, factorize :117, solve :1015,
solveLeastNorm_1 :1052, ObjectiveSensitivity :611, get_v :1560, get_x :1587, get_lexqr :1626,
getRank :1603, getTotalRank :1503) — one object is `batch` independent problems of one capacity.

Array conventions: a problem is the reference's column-major ``cap x (nVar+1)`` LOD, passed as a
C-ordered numpy array of shape ``(batch, nVar+1, cap)``.  Every compute call goes to the HIP
library; nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
from functools import partial

import numpy as np

from . import capi


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def _device_address(who, name, t, shape, dtype="torch.float64", raw_ok=False):
    """The address of an optional device argument `name` of the method `who`: None stays None, a raw address (anything without data_ptr(), where
    raw_ok) is taken as it is, everything else has to be a contiguous torch tensor of that dtype and shape."""
    if t is None:
        return None
    if raw_ok and not hasattr(t, "data_ptr"):
        return C.c_void_p(int(t))
    if not hasattr(t, "data_ptr") or str(t.dtype) != dtype or not t.is_contiguous() or tuple(t.shape) != shape:
        raise ValueError(f"{who}: {name} must be a contiguous {dtype.split('.')[1]} tensor of shape {shape}")
    return C.c_void_p(t.data_ptr())


def _leading_axis(shape, item_rank):
    """(lead, K) of an argument that holds K items of item_rank axes each, or one item without the leading axis: lead, (K,) or (), is what stands
    in front of an item's shape in every argument of the call.  K == 0 where `shape` has neither rank or no item: the caller refuses it."""
    if len(shape) == item_rank:
        return (), 1
    if len(shape) == item_rank + 1:
        return (int(shape[0]),), int(shape[0])
    return (), 0


class BatchedLexLSE:
    def __init__(self, batch: int, nVar: int, maxObjDim, device: int = 0):
        self._h = C.c_void_p()
        self.batch, self.nVar, self.device = int(batch), int(nVar), int(device)
        self.maxObjDim = np.ascontiguousarray(maxObjDim, dtype=np.uint32)
        self.nObj = int(self.maxObjDim.size)
        self.cap = int(self.maxObjDim.sum())
        capi.check(capi.lib().lexls_lse_create(C.byref(self._h), C.c_int(device), C.c_uint32(self.batch), C.c_uint32(self.nVar),
                                               C.c_uint32(self.nObj), _ptr(self.maxObjDim, C.c_uint32)))

    # ---- lifetime -------------------------------------------------------------------------------
    def close(self):
        if self._h:
            capi.lib().lexls_lse_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream: int):
        capi.check(capi.lib().lexls_lse_set_stream(self._h, C.c_void_p(hip_stream)))

    def synchronize(self):
        capi.check(capi.lib().lexls_lse_synchronize(self._h))

    # ---- problem definition ---------------------------------------------------------------------
    def setParameters(self, tol_linear_dependence: float = 1e-12):
        capi.check(capi.lib().lexls_lse_set_tolerance(self._h, C.c_double(tol_linear_dependence)))

    def setRegularization(self, regularization_type: int, factors=None, variable_factor: float = 0.0, cg_iterations: int = 10):
        """lexlse.h:1467/:1477: LexLS::RegularizationType (0 none, 1 Tikhonov, 2 Tikhonov by CGLS, 3 R, 4 R_NO_Z, 5 RT_NO_Z, 6 RT_NO_Z by CGLS, 8 Tikhonov_2, 9 test) and
        one factor per level ((nObj,)) or per problem and level ((batch, nObj))"""
        f = None if factors is None else np.ascontiguousarray(factors, dtype=np.float64)
        per = 1 if (f is not None and f.ndim == 2) else 0
        if f is not None and f.shape not in ((self.nObj,), (self.batch, self.nObj)):
            raise ValueError("factors must be (nObj,) or (batch, nObj)")
        capi.check(capi.lib().lexls_lse_set_cg_iterations(self._h, C.c_uint32(int(cg_iterations))))
        capi.check(capi.lib().lexls_lse_set_regularization(self._h, C.c_int(int(regularization_type)), _ptr(f, C.c_double) if f is not None else None,
                                                           C.c_int(per), C.c_double(variable_factor)))

    def setObjDim(self, dims):
        dims = np.ascontiguousarray(dims, dtype=np.uint32)
        per = 1 if dims.ndim == 2 else 0
        if per and dims.shape != (self.batch, self.nObj):
            raise ValueError("dims must be (nObj,) or (batch, nObj)")
        capi.check(capi.lib().lexls_lse_set_obj_dim(self._h, _ptr(dims, C.c_uint32), C.c_int(per)))

    def fixVariables(self, nfixed, index, value, ctr_type=None):
        if nfixed is None:
            capi.check(capi.lib().lexls_lse_set_fixed(self._h, None, None, None, None))
            return
        nfixed = np.ascontiguousarray(nfixed, np.uint32)
        index = np.ascontiguousarray(index, np.uint32)
        value = np.ascontiguousarray(value, np.float64)
        assert index.shape == (self.batch, self.nVar) and value.shape == (self.batch, self.nVar)
        ctr_type = None if ctr_type is None else np.ascontiguousarray(ctr_type, np.uint8)
        capi.check(capi.lib().lexls_lse_set_fixed(self._h, _ptr(nfixed, C.c_uint32), _ptr(index, C.c_uint32), _ptr(value, C.c_double),
                                                  _ptr(ctr_type, C.c_uint8)))

    def setCtrType(self, types):
        types = np.ascontiguousarray(types, np.uint8)
        assert types.shape == (self.batch, self.cap)
        capi.check(capi.lib().lexls_lse_set_ctr_type(self._h, _ptr(types, C.c_uint8)))

    def set_skip(self, mask):
        """lexls_lse_set_skip: mask (batch,) uint8 — problems whose byte is non-zero are left untouched by the following factorize /
        factorize_solve calls (their previous results stay valid: x, pivots, ranks, the kept factor, the accuracy guard's report); None
        clears the mask.  Holds for problems whose dimensions and fixed variables are those of the run their results come from."""
        if mask is None:
            capi.check(capi.lib().lexls_lse_set_skip(self._h, None))
            return
        mask = np.ascontiguousarray(mask, np.uint8)
        if mask.shape != (self.batch,):
            raise ValueError(f"mask must have shape {(self.batch,)}, got {mask.shape}")
        capi.check(capi.lib().lexls_lse_set_skip(self._h, _ptr(mask, C.c_uint8)))

    def setProblem(self, lod):
        """lod: host array (batch, nVar+1, cap); copied to the device."""
        lod = np.ascontiguousarray(lod, np.float64)
        if lod.shape != (self.batch, self.nVar + 1, self.cap):
            raise ValueError(f"lod must have shape {(self.batch, self.nVar + 1, self.cap)}, got {lod.shape}")
        capi.check(capi.lib().lexls_lse_set_problem_host(self._h, _ptr(lod, C.c_double)))

    def setProblemDevice(self, device_ptr: int):
        """Bind a device buffer (e.g. torch_tensor.data_ptr()) holding batch x cap x (nVar+1) doubles as the input: zero-copy, read in the
        handle's stream, never written.  The address must be a multiple of 8 bytes (LexlsError otherwise, the handle keeps what it had);
        lqr_qtol's uniform form and lqr_mfma need 16 and give way to the bit-exact kernel on a pointer that is 8 mod 16."""
        capi.check(capi.lib().lexls_lse_set_problem_device(self._h, C.c_void_p(device_ptr)))

    # ---- one copy each way per round (lock-step active-set batches) -----------------------------
    _ROUND_FIELDS = ("in_bytes", "dims", "nfixed", "fixed_idx", "fixed_val", "skip", "obj_index", "row_src", "row_ld", "fixed_type", "ctr_type",
                     "out_bytes", "x", "total_rank", "found", "max_abs")

    def round_layout(self) -> dict:
        """byte offsets of the per-round arrays inside the handle's two device slabs (lexls_lse_round_layout)"""
        lay = (C.c_uint64 * len(self._ROUND_FIELDS))()
        capi.check(capi.lib().lexls_lse_round_layout(self._h, lay))
        return dict(zip(self._ROUND_FIELDS, [int(v) for v in lay]))

    def round_views(self, block: np.ndarray) -> dict:
        """typed numpy views of an in-slab-shaped uint8 block (round_layout()['in_bytes'] bytes)"""
        L, B, n, cap = self.round_layout(), self.batch, self.nVar, self.cap
        def view(off, dtype, shape):
            count = int(np.prod(shape))
            return block[off:off + count * np.dtype(dtype).itemsize].view(dtype).reshape(shape)
        return dict(dims=view(L["dims"], np.uint32, (B, self.nObj)), nfixed=view(L["nfixed"], np.uint32, (B,)),
                    fixed_idx=view(L["fixed_idx"], np.uint32, (B, n)), fixed_val=view(L["fixed_val"], np.float64, (B, n)),
                    skip=view(L["skip"], np.uint8, (B,)), obj_index=view(L["obj_index"], np.int32, (B,)),
                    row_src=view(L["row_src"], np.uint32, (B, cap)), row_ld=view(L["row_ld"], np.uint32, (B, cap)),
                    fixed_type=view(L["fixed_type"], np.uint8, (B, n)), ctr_type=view(L["ctr_type"], np.uint8, (B, cap)))

    def upload_round(self, block: np.ndarray, gather: bool = False):
        assert block.dtype == np.uint8 and block.flags.c_contiguous and block.size == self.round_layout()["in_bytes"]
        capi.check(capi.lib().lexls_lse_upload_round(self._h, block.ctypes.data_as(C.c_void_p), C.c_int(1 if gather else 0)))

    def download_round(self, with_types: bool = True) -> dict:
        L, B, n, cap = self.round_layout(), self.batch, self.nVar, self.cap
        out = np.zeros(L["out_bytes"], np.uint8)
        types = np.zeros(L["in_bytes"] - L["fixed_type"], np.uint8) if with_types else None
        capi.check(capi.lib().lexls_lse_download_round(self._h, out.ctypes.data_as(C.c_void_p), types.ctypes.data_as(C.c_void_p) if with_types else None))
        r = dict(x=out[L["x"]:L["x"] + 8 * B * n].view(np.float64).reshape(B, n), total_rank=out[L["total_rank"]:L["total_rank"] + 4 * B].view(np.uint32),
                 found=out[L["found"]:L["found"] + 12 * B].view(np.int32).reshape(B, 3), max_abs=out[L["max_abs"]:L["max_abs"] + 8 * B].view(np.float64))
        if with_types:
            o = L["ctr_type"] - L["fixed_type"]
            r["fixed_type"] = types[:B * n].reshape(B, n)
            r["ctr_type"] = types[o:o + B * cap].reshape(B, cap)
        return r

    def sensitivity_resident(self, tol_wrong_sign_lambda=1e-8, tol_correct_sign_lambda=1e-12):
        """ObjectiveSensitivity with the per-problem objective indices uploaded by upload_round"""
        capi.check(capi.lib().lexls_lse_sensitivity_resident(self._h, C.c_double(tol_wrong_sign_lambda), C.c_double(tol_correct_sign_lambda)))

    # ---- hot path -------------------------------------------------------------------------------
    def factorize(self):
        capi.check(capi.lib().lexls_lse_factorize(self._h))

    def solve(self):
        capi.check(capi.lib().lexls_lse_solve(self._h))

    def factorize_solve(self, keep_factor: bool = True):
        capi.check(capi.lib().lexls_lse_factorize_solve(self._h, C.c_int(1 if keep_factor else 0)))

    def solveLeastNorm_1(self):
        capi.check(capi.lib().lexls_lse_solve_least_norm(self._h))

    def solveLeastNorm_3(self):
        """lexlse.h:1222-1277: least-norm solution from the null-space basis of the Tikhonov family"""
        capi.check(capi.lib().lexls_lse_solve_least_norm_3(self._h))

    def solveLeastNorm_2(self):
        """lexlse.h:1138-1213: least-norm solution through the normal equations of the free variables"""
        capi.check(capi.lib().lexls_lse_solve_least_norm_2(self._h))

    def setSensitivityScan(self, on: bool):
        """while on, ObjectiveSensitivity(level) goes on through the following levels until one reports a wrong-sign multiplier or the last
        level is done (LexLSI's removal search, lexlsi.h:1121-1132, in one launch); outputs are those of the level it stopped at"""
        capi.check(capi.lib().lexls_lse_set_sensitivity_scan(self._h, C.c_int(1 if on else 0)))

    def ObjectiveSensitivity(self, ObjIndex, tol_wrong_sign_lambda=1e-8, tol_correct_sign_lambda=1e-12):
        """ObjIndex: int (all problems) or per-problem int32 array (negative = skip). Returns (found, ctr, obj, maxAbs)."""
        if np.isscalar(ObjIndex):
            capi.check(capi.lib().lexls_lse_sensitivity(self._h, None, C.c_int32(int(ObjIndex)), C.c_double(tol_wrong_sign_lambda),
                                                        C.c_double(tol_correct_sign_lambda)))
        else:
            oi = np.ascontiguousarray(ObjIndex, np.int32)
            assert oi.shape == (self.batch,)
            capi.check(capi.lib().lexls_lse_sensitivity(self._h, _ptr(oi, C.c_int32), C.c_int32(0), C.c_double(tol_wrong_sign_lambda),
                                                        C.c_double(tol_correct_sign_lambda)))
        sens = np.zeros((self.batch, 3), np.int32)
        maxabs = np.zeros(self.batch)
        capi.check(capi.lib().lexls_lse_get_sensitivity(self._h, _ptr(sens, C.c_int32), _ptr(maxabs, C.c_double)))
        return sens[:, 0].astype(bool), sens[:, 1], sens[:, 2], maxabs

    def sensitivity_collect(self, ObjIndex, tol_wrong_sign_lambda=1e-8, tol_correct_sign_lambda=1e-12):
        """The collecting overload ObjectiveSensitivity(ObjIndex, tolW, tolC, ctr_wrong_sign) (lexlse.h:511-602, deactivate_first_wrong_sign):
        every wrong-sign multiplier instead of the most negative one.  ObjIndex: int (all problems), per-problem int32 array (negative =
        skip) or None (the indices upload_round left on the device).  Returns (non_empty, entries, obj): per problem whether the set is
        non-empty, its size and the objective the search stopped at; the set itself: wrong_sign()."""
        lib = capi.lib()
        if ObjIndex is None:
            capi.check(lib.lexls_lse_sensitivity_collect_resident(self._h, C.c_double(tol_wrong_sign_lambda), C.c_double(tol_correct_sign_lambda)))
        elif np.isscalar(ObjIndex):
            capi.check(lib.lexls_lse_sensitivity_collect(self._h, None, C.c_int32(int(ObjIndex)), C.c_double(tol_wrong_sign_lambda), C.c_double(tol_correct_sign_lambda)))
        else:
            oi = np.ascontiguousarray(ObjIndex, np.int32)
            assert oi.shape == (self.batch,)
            capi.check(lib.lexls_lse_sensitivity_collect(self._h, _ptr(oi, C.c_int32), C.c_int32(0), C.c_double(tol_wrong_sign_lambda), C.c_double(tol_correct_sign_lambda)))
        sens = np.zeros((self.batch, 3), np.int32)
        capi.check(lib.lexls_lse_get_sensitivity(self._h, _ptr(sens, C.c_int32), None))
        return sens[:, 0].astype(bool), sens[:, 1], sens[:, 2]

    def wrong_sign(self):
        """the set of the last sensitivity_collect call, (batch, nVar + cap) uint8: columns [0, nVar) the fixed variables in fixVariable order,
        then the constraint rows in LOD order; 1 where the reference pushes a ConstraintInfo"""
        m = np.zeros((self.batch, self.nVar + self.cap), np.uint8)
        capi.check(capi.lib().lexls_lse_get_wrong_sign(self._h, _ptr(m, C.c_uint8)))
        return m

    # ---- results --------------------------------------------------------------------------------
    def get_x(self):
        x = np.zeros((self.batch, self.nVar))
        capi.check(capi.lib().lexls_lse_get_x(self._h, _ptr(x, C.c_double)))
        return x

    def get_lexqr(self):
        f = np.zeros((self.batch, self.nVar + 1, self.cap))
        capi.check(capi.lib().lexls_lse_get_factor(self._h, _ptr(f, C.c_double)))
        return f

    def get_hh_scalars(self):
        h = np.zeros((self.batch, self.cap))
        capi.check(capi.lib().lexls_lse_get_hh_scalars(self._h, _ptr(h, C.c_double)))
        return h

    def get_column_permutations(self):
        p = np.zeros((self.batch, self.nVar), np.uint32)
        capi.check(capi.lib().lexls_lse_get_permutation(self._h, _ptr(p, C.c_uint32)))
        return p

    def getRanks(self):
        r = np.zeros((self.batch, self.nObj), np.uint32)
        fc = np.zeros((self.batch, self.nObj), np.uint32)
        tr = np.zeros(self.batch, np.uint32)
        capi.check(capi.lib().lexls_lse_get_ranks(self._h, _ptr(r, C.c_uint32), _ptr(fc, C.c_uint32), _ptr(tr, C.c_uint32)))
        return r, fc, tr

    def get_v(self):
        capi.check(capi.lib().lexls_lse_residual(self._h))
        v = np.zeros((self.batch, self.cap))
        capi.check(capi.lib().lexls_lse_get_v(self._h, _ptr(v, C.c_double)))
        return v

    def get_mu(self):
        """(X_mu, X_mu_rhs, residual_mu) of REGULARIZATION_TIKHONOV_1 (lexlse.h:1636-1650): (batch, nObj, nVar) twice — row k is the
        reference's column k — and (batch, cap)."""
        xm = np.zeros((self.batch, self.nObj, self.nVar))
        xr = np.zeros((self.batch, self.nObj, self.nVar))
        rm = np.zeros((self.batch, self.cap))
        capi.check(capi.lib().lexls_lse_get_mu(self._h, _ptr(xm, C.c_double), _ptr(xr, C.c_double), _ptr(rm, C.c_double)))
        return xm, xr, rm

    def getWorkspace(self):
        """[lambda_fixed; lambda] of the last ObjectiveSensitivity call, shape (batch, nVar+cap)."""
        lam = np.zeros((self.batch, self.nVar + self.cap))
        capi.check(capi.lib().lexls_lse_get_lambda(self._h, _ptr(lam, C.c_double)))
        return lam

    def multipliers(self):
        """every objective's multipliers on the current factor (lexls_lse_multipliers + lexls_lse_get_multipliers): (batch, nObj, nVar+cap),
        row k of problem b = getWorkspace() after ObjectiveSensitivity(k) — zero from nfixed + dims[0] + ... + dims[k] on"""
        capi.check(capi.lib().lexls_lse_multipliers(self._h))
        L = np.zeros((self.batch, self.nObj, self.nVar + self.cap))
        capi.check(capi.lib().lexls_lse_get_multipliers(self._h, _ptr(L, C.c_double)))
        return L

    # ---- adjoint of the solve (A held fixed) ------------------------------------------------------
    def set_adjoint_regularized(self, on: bool = True):
        """lexls_lse_set_adjoint_regularized: let solve_adjoint and solve_adjoint_device answer after a damped factorization (regularization
        type 1, 3, 4, 5, 8 or 9 with variable_factor == 0).  Off by default: they then raise LEXLS_ERR_UNSUPPORTED after every regularized
        factorization, as they always did."""
        capi.check(capi.lib().lexls_lse_set_adjoint_regularized(self._h, C.c_int(1 if on else 0)))
        self._adj_reg = bool(on)

    def set_adjoint_regularized_multi(self, on: bool = True):
        """lexls_lse_set_adjoint_regularized_multi: let solve_adjoint_multi, solve_adjoint_multi_device and jacobian_device() answer after a damped
        factorization (regularization type 1, 3, 4, 5, 8 or 9 with variable_factor == 0): M_reg^T g_c and N_reg^T g_c for every cotangent, the
        factors held fixed.  Off by default, and independent of set_adjoint_regularized(): they then raise LEXLS_ERR_UNSUPPORTED after every
        regularized factorization, as they always did."""
        capi.check(capi.lib().lexls_lse_set_adjoint_regularized_multi(self._h, C.c_int(1 if on else 0)))
        self._adj_reg_multi = bool(on)

    def _one_cotangent_on_the_multi_entry(self):
        """K == 1 goes to the single-cotangent entry (one live lane of the multi-cotangent kernel is slower) — unless this handle switched the
        damped adjoint on for the multi calls alone: the single entry would refuse a damped factor then"""
        return getattr(self, "_adj_reg_multi", False) and not getattr(self, "_adj_reg", False)

    def solve_adjoint(self, g):
        """lexls_lse_solve_adjoint + lexls_lse_get_adjoint: for fixed A the basic solution is affine in the right-hand sides and the fixed
        values, x = M b + N x_fixed; with g = dloss/dx, (batch, nVar) in the order of get_x(), returns (grad_rhs, grad_fixed) = (M^T g, N^T g)
        as numpy arrays: (batch, cap) in LOD row order (zero behind a problem's own rows) and (batch, nVar), entry j < nfixed the fixed variable
        of slot j in fixVariable order, zero from nfixed on.  Needs a kept factor: unregularized, or (after set_adjoint_regularized()) regularized with type 1, 3, 4, 5, 8 or 9 and
        variable_factor == 0 — then M and N are those of the damped solve, the factors held fixed as A is (no gradient with respect to them);
        types 2, 6, 7 and a variable factor raise (LEXLS_ERR_UNSUPPORTED).  No derivatives with respect to A."""
        g = np.ascontiguousarray(g, np.float64)
        if g.shape != (self.batch, self.nVar):
            raise ValueError(f"g must have shape {(self.batch, self.nVar)}, got {g.shape}")
        capi.check(capi.lib().lexls_lse_solve_adjoint(self._h, _ptr(g, C.c_double)))
        grad_rhs = np.zeros((self.batch, self.cap))
        grad_fixed = np.zeros((self.batch, self.nVar))
        capi.check(capi.lib().lexls_lse_get_adjoint(self._h, _ptr(grad_rhs, C.c_double), _ptr(grad_fixed, C.c_double)))
        return grad_rhs, grad_fixed

    def solve_adjoint_device(self, g, grad_rhs, grad_fixed=None):
        """lexls_lse_solve_adjoint_device: g (batch, nVar), grad_rhs (batch, cap) and grad_fixed (batch, nVar; None: not wanted) in device memory —
        contiguous float64 torch tensors (anything with data_ptr()) or raw addresses.  Only enqueued in the handle's stream (set_stream): g has
        to be complete in stream order, nothing is waited for.  Serves the same factors as solve_adjoint (regularization types 1, 3, 4, 5, 8, 9)."""
        address = partial(_device_address, "solve_adjoint_device", raw_ok=True)
        capi.check(capi.lib().lexls_lse_solve_adjoint_device(self._h, address("g", g, (self.batch, self.nVar)),
                                                              address("grad_rhs", grad_rhs, (self.batch, self.cap)),
                                                              address("grad_fixed", grad_fixed, (self.batch, self.nVar))))

    # ---- the same adjoint for many cotangents per problem in one pass (lane = cotangent) --------------
    def solve_adjoint_multi(self, G):
        """lexls_lse_solve_adjoint_multi + lexls_lse_get_adjoint_multi: G (batch, K, nVar), K cotangents per problem in the order of get_x().
        Returns (grad_rhs (batch, K, cap), grad_fixed (batch, K, nVar)), row c what solve_adjoint(G[:, c]) returns (tolerance contract); a
        cotangent's bits do not depend on K, on its position or on its neighbours.  One cotangent goes to the single-cotangent entry (to the multi
        entry where set_adjoint_regularized_multi() alone is on).  A damped factor needs set_adjoint_regularized_multi()."""
        G = np.ascontiguousarray(G, np.float64)
        if G.ndim != 3 or G.shape[0] != self.batch or G.shape[1] == 0 or G.shape[2] != self.nVar:
            raise ValueError(f"G must have shape ({self.batch}, K >= 1, {self.nVar}), got {G.shape}")
        K = G.shape[1]
        if K == 1 and not self._one_cotangent_on_the_multi_entry():
            grad_rhs, grad_fixed = self.solve_adjoint(G[:, 0, :])
            return grad_rhs[:, None, :], grad_fixed[:, None, :]
        capi.check(capi.lib().lexls_lse_solve_adjoint_multi(self._h, _ptr(G, C.c_double), K))
        grad_rhs = np.zeros((self.batch, K, self.cap))
        grad_fixed = np.zeros((self.batch, K, self.nVar))
        capi.check(capi.lib().lexls_lse_get_adjoint_multi(self._h, _ptr(grad_rhs, C.c_double), _ptr(grad_fixed, C.c_double)))
        return grad_rhs, grad_fixed

    def solve_adjoint_multi_device(self, G, grad_rhs, grad_fixed=None):
        """lexls_lse_solve_adjoint_multi_device: G (batch, K, nVar), grad_rhs (batch, K, cap) and grad_fixed (batch, K, nVar; None: not wanted) in
        device memory, contiguous float64 torch tensors.  Only enqueued in the handle's stream.  K == 1 goes to solve_adjoint_device (the
        single-cotangent kernel: one live lane of the multi-cotangent one would be slower)."""
        if not hasattr(G, "data_ptr") or G.dim() != 3 or G.shape[1] == 0:
            raise ValueError("solve_adjoint_multi_device: G must be a tensor of shape (batch, K >= 1, nVar)")
        K = int(G.shape[1])
        address = partial(_device_address, "solve_adjoint_multi_device")
        args = (address("G", G, (self.batch, K, self.nVar)), address("grad_rhs", grad_rhs, (self.batch, K, self.cap)),
                address("grad_fixed", grad_fixed, (self.batch, K, self.nVar)))
        if K == 1 and not self._one_cotangent_on_the_multi_entry():
            capi.check(capi.lib().lexls_lse_solve_adjoint_device(self._h, *args))
        else:
            capi.check(capi.lib().lexls_lse_solve_adjoint_multi_device(self._h, args[0], K, args[1], args[2]))

    # ---- gradient with respect to the matrix (rank-stable problems) ---------------------------------
    def solve_adjoint_matrix(self, g):
        """lexls_lse_solve_adjoint_matrix + lexls_lse_get_adjoint_matrix: g = dloss/dx, (batch, nVar) in the order of get_x().  Returns
        (grad_lod, differentiable): grad_lod (batch, nVar + 1, cap) in the layout of the problem data — grad_lod[b, j, i] the gradient of entry
        (row i, column j) of A for j < nVar, grad_lod[b, nVar] the gradient of the right-hand side, zero behind a problem's own rows — and
        differentiable (batch,) uint8: 1 where the problem is rank-stable (rank_k == min(dim_k, nVar - Fc_k) for every level, or every variable
        fixed), 0 where it is not and no derivative exists; there grad_lod[b] is entirely zero.  Needs a kept, unregularized factor and its x
        (factorize_solve(keep_factor=True), or factorize() + solve())."""
        g = np.ascontiguousarray(g, np.float64)
        if g.shape != (self.batch, self.nVar):
            raise ValueError(f"g must have shape {(self.batch, self.nVar)}, got {g.shape}")
        capi.check(capi.lib().lexls_lse_solve_adjoint_matrix(self._h, _ptr(g, C.c_double)))
        grad_lod = np.zeros((self.batch, self.nVar + 1, self.cap))
        differentiable = np.zeros(self.batch, np.uint8)
        capi.check(capi.lib().lexls_lse_get_adjoint_matrix(self._h, _ptr(grad_lod, C.c_double), _ptr(differentiable, C.c_uint8)))
        return grad_lod, differentiable

    def solve_adjoint_matrix_device(self, g, grad_lod, differentiable=None):
        """lexls_lse_solve_adjoint_matrix_device: g (batch, nVar) float64, grad_lod (batch, nVar + 1, cap) float64 and differentiable (batch,)
        uint8 (None: not wanted) in device memory — contiguous torch tensors or raw addresses.  Only enqueued in the handle's stream (set_stream):
        g has to be complete in stream order, nothing is waited for."""
        address = partial(_device_address, "solve_adjoint_matrix_device", raw_ok=True)
        capi.check(capi.lib().lexls_lse_solve_adjoint_matrix_device(self._h, address("g", g, (self.batch, self.nVar)),
                                                                     address("grad_lod", grad_lod, (self.batch, self.nVar + 1, self.cap)),
                                                                     address("differentiable", differentiable, (self.batch,), "torch.uint8")))

    # ---- forward-mode tangents of the solve with respect to its data (rank-stable problems) ----------
    def solve_tangent(self, dlod, dfixed=None):
        """lexls_lse_solve_tangent + lexls_lse_get_tangent: dlod (K, batch, nVar + 1, cap), K directions d[A | b] in the layout of the problem
        data (rows behind a problem's own are not read), or (batch, nVar + 1, cap) for one; dfixed (K, batch, nVar) / (batch, nVar), slot j <
        nfixed the tangent of the j-th fixed value (None: zeros).  Returns (dx, differentiable): dx (K, batch, nVar) — (batch, nVar) for a
        single direction given without the leading axis — in the order of get_x(), and differentiable (batch,) uint8, the flags of
        solve_adjoint_matrix; where the flag is 0 the problem's rows of dx are exact zeros.  Needs what solve_adjoint_matrix needs."""
        dlod = np.ascontiguousarray(dlod, np.float64)
        lead, K = _leading_axis(dlod.shape, 3)
        single = K == 1 and not lead
        if single:
            dlod = dlod[None]
        if K == 0 or dlod.shape[1:] != (self.batch, self.nVar + 1, self.cap):
            raise ValueError(f"dlod must have shape (K >= 1, {self.batch}, {self.nVar + 1}, {self.cap}) or lack the leading axis, got {dlod.shape}")
        if dfixed is not None:
            dfixed = np.ascontiguousarray(dfixed, np.float64).reshape((K, self.batch, self.nVar))
        capi.check(capi.lib().lexls_lse_solve_tangent(self._h, _ptr(dlod, C.c_double), None if dfixed is None else _ptr(dfixed, C.c_double), K))
        dx = np.zeros((K, self.batch, self.nVar))
        differentiable = np.zeros(self.batch, np.uint8)
        capi.check(capi.lib().lexls_lse_get_tangent(self._h, _ptr(dx, C.c_double), _ptr(differentiable, C.c_uint8)))
        return (dx[0] if single else dx), differentiable

    def solve_tangent_device(self, dlod, dx, dfixed=None, differentiable=None):
        """lexls_lse_solve_tangent_device: dlod (K, batch, nVar + 1, cap), dx (K, batch, nVar), dfixed (K, batch, nVar; None: zeros) float64 and
        differentiable (batch,) uint8 (None: not wanted) in device memory, contiguous torch tensors; a single direction may lack the leading
        axis in all three.  Only enqueued in the handle's stream (set_stream): the directions have to be complete in stream order."""
        if not hasattr(dlod, "data_ptr") or dlod.dim() not in (3, 4):
            raise ValueError("solve_tangent_device: dlod must be a tensor of shape (K >= 1, batch, nVar + 1, cap) or (batch, nVar + 1, cap)")
        lead, K = _leading_axis(dlod.shape, 3)
        if K == 0:
            raise ValueError("solve_tangent_device: K == 0")
        address = partial(_device_address, "solve_tangent_device")
        capi.check(capi.lib().lexls_lse_solve_tangent_device(self._h, address("dlod", dlod, lead + (self.batch, self.nVar + 1, self.cap)),
                                                              address("dfixed", dfixed, lead + (self.batch, self.nVar)), K,
                                                              address("dx", dx, lead + (self.batch, self.nVar)),
                                                              address("differentiable", differentiable, (self.batch,), "torch.uint8")))

    # ---- new right-hand sides on the kept factor (every problem; plain and damped factors) ----------
    def solve_rhs(self, rhs, fixed=None):
        """lexls_lse_solve_rhs + lexls_lse_get_solve_rhs: rhs (K, batch, cap), K right-hand sides per problem in LOD row order (rows behind a
        problem's own are not read), or (batch, cap) for one; fixed (K, batch, nVar) / (batch, nVar), slot j < nfixed the j-th fixed value
        (None: the values the handle holds).  Returns x (K, batch, nVar) — (batch, nVar) for a 2-D rhs — in the order of get_x(): what
        factorize_solve() gives for the same matrices under that right-hand side and those fixed values, within the tolerance contract.
        Needs a kept factor only (factorize() is enough); after setRegularization: types 1, 3, 4, 5, 8, 9 with constant factors."""
        rhs = np.ascontiguousarray(rhs, np.float64)
        lead, K = _leading_axis(rhs.shape, 2)
        single = K == 1 and not lead
        if single:
            rhs = rhs[None]
        if K == 0 or rhs.shape[1:] != (self.batch, self.cap):
            raise ValueError(f"rhs must have shape (K >= 1, {self.batch}, {self.cap}) or lack the leading axis, got {rhs.shape}")
        if fixed is not None:
            fixed = np.ascontiguousarray(fixed, np.float64).reshape((K, self.batch, self.nVar))
        capi.check(capi.lib().lexls_lse_solve_rhs(self._h, _ptr(rhs, C.c_double), None if fixed is None else _ptr(fixed, C.c_double), K))
        x = np.zeros((K, self.batch, self.nVar))
        capi.check(capi.lib().lexls_lse_get_solve_rhs(self._h, _ptr(x, C.c_double)))
        return x[0] if single else x

    def solve_rhs_device(self, rhs, x, fixed=None):
        """lexls_lse_solve_rhs_device: rhs (K, batch, cap), x (K, batch, nVar), fixed (K, batch, nVar; None: the handle's values) float64 in
        device memory, contiguous torch tensors; a single right-hand side may lack the leading axis in all three.  Only enqueued in the
        handle's stream (set_stream): the inputs have to be complete in stream order."""
        if not hasattr(rhs, "data_ptr") or rhs.dim() not in (2, 3):
            raise ValueError("solve_rhs_device: rhs must be a tensor of shape (K >= 1, batch, cap) or (batch, cap)")
        lead, K = _leading_axis(rhs.shape, 2)
        if K == 0:
            raise ValueError("solve_rhs_device: K == 0")
        address = partial(_device_address, "solve_rhs_device")
        capi.check(capi.lib().lexls_lse_solve_rhs_device(self._h, address("rhs", rhs, lead + (self.batch, self.cap)),
                                                          address("fixed", fixed, lead + (self.batch, self.nVar)), K,
                                                          address("x", x, lead + (self.batch, self.nVar))))

    # ---- residuals of new right-hand sides on the kept factor (every problem; undamped factors) ----------
    def residual_rhs(self, rhs, fixed=None):
        """lexls_lse_residual_rhs + lexls_lse_get_residual_rhs: rhs and fixed as for solve_rhs().  Returns (v, cost): v (K, batch, cap), per
        right-hand side what residual() + get_v() give for the same matrices under that right-hand side and those fixed values (LOD row order,
        zeros behind a problem's own rows), within the tolerance contract; cost (K, batch, nObj), the sum of squares of each level's rows of v
        (exactly 0.0 for a level of full row rank).  Both lack the leading axis for a 2-D rhs.  Needs a kept, undamped factor only."""
        rhs = np.ascontiguousarray(rhs, np.float64)
        lead, K = _leading_axis(rhs.shape, 2)
        single = K == 1 and not lead
        if single:
            rhs = rhs[None]
        if K == 0 or rhs.shape[1:] != (self.batch, self.cap):
            raise ValueError(f"rhs must have shape (K >= 1, {self.batch}, {self.cap}) or lack the leading axis, got {rhs.shape}")
        if fixed is not None:
            fixed = np.ascontiguousarray(fixed, np.float64).reshape((K, self.batch, self.nVar))
        capi.check(capi.lib().lexls_lse_residual_rhs(self._h, _ptr(rhs, C.c_double), None if fixed is None else _ptr(fixed, C.c_double), K))
        v, cost = np.zeros((K, self.batch, self.cap)), np.zeros((K, self.batch, self.nObj))
        capi.check(capi.lib().lexls_lse_get_residual_rhs(self._h, _ptr(v, C.c_double), _ptr(cost, C.c_double)))
        return (v[0], cost[0]) if single else (v, cost)

    def residual_rhs_device(self, rhs, v=None, cost=None, x=None, fixed=None):
        """lexls_lse_residual_rhs_device: rhs (K, batch, cap), fixed (K, batch, nVar; None: the handle's values), and the outputs v (K, batch, cap),
        cost (K, batch, nObj), x (K, batch, nVar: solve_rhs_device()'s, bit for bit) — any of the three may be None, not all — float64 in device
        memory, contiguous torch tensors; a single right-hand side may lack the leading axis in all of them.  Only enqueued in the handle's
        stream (set_stream): the inputs have to be complete in stream order."""
        if not hasattr(rhs, "data_ptr") or rhs.dim() not in (2, 3):
            raise ValueError("residual_rhs_device: rhs must be a tensor of shape (K >= 1, batch, cap) or (batch, cap)")
        lead, K = _leading_axis(rhs.shape, 2)
        if K == 0:
            raise ValueError("residual_rhs_device: K == 0")
        address = partial(_device_address, "residual_rhs_device")
        capi.check(capi.lib().lexls_lse_residual_rhs_device(self._h, address("rhs", rhs, lead + (self.batch, self.cap)),
                                                             address("fixed", fixed, lead + (self.batch, self.nVar)), K,
                                                             address("x", x, lead + (self.batch, self.nVar)), address("v", v, lead + (self.batch, self.cap)),
                                                             address("cost", cost, lead + (self.batch, self.nObj))))

    def jacobian_device(self):
        """(dx_db (batch, nVar, cap), dx_dfixed (batch, nVar, nVar)) of the kept factor as torch tensors on the handle's device: the identity
        cotangents are built there and go through solve_adjoint_multi_device, so dx_db[b, i, r] = d x_i / d b_r (LOD row order) and
        dx_dfixed[b, i, j] = d x_i / d x_fixed_j (fixVariable order, zero from nfixed on).  Enqueued in the handle's stream, not waited for.
        After a damped factorization on a handle with set_adjoint_regularized_multi(): M_reg and N_reg of the damped solve."""
        import torch
        dev = torch.device("cuda", self.device)
        G = torch.eye(self.nVar, dtype=torch.float64, device=dev).expand(self.batch, self.nVar, self.nVar).contiguous()
        dx_db = torch.empty((self.batch, self.nVar, self.cap), dtype=torch.float64, device=dev)
        dx_dfixed = torch.empty((self.batch, self.nVar, self.nVar), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()  # the cotangents are complete before the handle's stream reads them
        self.solve_adjoint_multi_device(G, dx_db, dx_dfixed)
        return dx_db, dx_dfixed

    def getCtrType(self):
        t = np.zeros((self.batch, self.cap), np.uint8)
        capi.check(capi.lib().lexls_lse_get_ctr_type(self._h, _ptr(t, C.c_uint8)))
        return t

    def getFixedType(self):
        """activation types of the fixed variables incl. the CORRECT_SIGN_OF_LAMBDA marks, (batch, nVar)"""
        t = np.zeros((self.batch, self.nVar), np.uint8)
        capi.check(capi.lib().lexls_lse_get_fixed_type(self._h, _ptr(t, C.c_uint8)))
        return t

    def device_ptr(self, name: str) -> int:
        p = C.c_void_p()
        capi.check(capi.lib().lexls_lse_device_ptr(self._h, C.c_int(capi.ARRAY[name]), C.byref(p)))
        return int(p.value)

    def set_prefix_reuse(self, enable: bool = True):
        """lexls_lse_set_prefix_reuse: factor-keeping factorizations by the register-resident wave kernel leave what a later one needs to
        read unchanged leading levels back instead of factorizing them (the reference has no such mechanism, README.md:14)"""
        capi.check(capi.lib().lexls_lse_set_prefix_reuse(self._h, C.c_int(1 if enable else 0)))

    def prefix_reuse_ready(self) -> bool:
        return bool(capi.lib().lexls_lse_prefix_reuse_ready(self._h))

    def set_resume_levels(self, levels):
        """levels[b] = number of leading levels of problem b that are unchanged since its previous factorization (consumed by the next one)"""
        lv = np.ascontiguousarray(np.broadcast_to(np.asarray(levels, np.int32), (self.batch,)))
        capi.check(capi.lib().lexls_lse_set_resume_levels(self._h, lv.ctypes.data_as(C.c_void_p)))

    def set_kernel_policy(self, policy: int):
        """diagnostics (lexls_lse_set_kernel_policy): 0 automatic dispatch, 1 generic kernel only, 2 never the left-looking wave kernel,
        3 the left-looking wave kernel whenever the shape allows it, 4 the bit-exact four-problems-per-wavefront kernel, 5 bit-exact everywhere,
        6 the tolerance-contract kernel lqr_qtol wherever it serves (levels of exactly 12 or exactly 8 rows), 7 / 8 / 9 lqr_mfma,
        10 as 6 plus lqr_qtol's ragged instantiations: x-only solves whose levels have at most 12 rows each, per-problem dimensions (setObjDim
        with a (batch, nObj) array), empty levels included; same tolerance contract (include/lexls_hip.h)"""
        capi.check(capi.lib().lexls_lse_set_kernel_policy(self._h, C.c_int(int(policy))))

    def last_kernel(self) -> str:
        return capi.lib().lexls_lse_last_kernel(self._h).decode()

    def last_consumer_kernel(self) -> str:
        """the kernel variant that served the last post-factorization call — solve, get_v, ObjectiveSensitivity / sensitivity_collect,
        multipliers, solveLeastNorm_* — (lexls_lse_last_consumer_kernel): "solve_generic<256>", "sensitivity_sweep<12>",
        "sensitivity<64,staged>", "multipliers<per-objective>", "leastnorm_2<64>", ...; "" when none has launched on the current factor"""
        buf = C.create_string_buffer(64)
        capi.check(capi.lib().lexls_lse_last_consumer_kernel(self._h, buf, C.c_size_t(len(buf))))
        return buf.value.decode()

    def last_large_levels(self):
        """(in_launch, redone) of the last factorization (lexls_lse_last_large_levels): levels whose pivots lqr_large<step-per-pivot,mfma> ran
        inside ONE launch, and levels that launch gave up and the host redid with a launch per pivot; (0, 0) on every other kernel, for a
        batch, under LEXLS_LARGE_PERSIST=0 and where no form of the launch fits the device"""
        a, r = C.c_uint32(0), C.c_uint32(0)
        capi.check(capi.lib().lexls_lse_last_large_levels(self._h, C.byref(a), C.byref(r)))
        return int(a.value), int(r.value)

    def last_reg_placement(self):
        """(window_order, basis_in_lds) of the last factorization (lexls_lse_last_reg_placement): the order of the LDS window the regularized
        wave kernel gave its routines' work matrix (0: none) and whether it kept the null-space basis in LDS; (0, False) on every other kernel
        and without regularization"""
        w, b = C.c_uint32(0), C.c_uint32(0)
        capi.check(capi.lib().lexls_lse_last_reg_placement(self._h, C.byref(w), C.byref(b)))
        return int(w.value), bool(b.value)

    def set_accuracy_guard(self, mode: int, threshold: float = 0.0):
        """lexls_lse_set_accuracy_guard: 0 off (default), 1 report, 2 report and re-solve the flagged problems on the bit-exact kernel
        (include/lexls_hip.h, policy comment); threshold <= 0: the calibrated default"""
        capi.check(capi.lib().lexls_lse_set_accuracy_guard(self._h, int(mode), float(threshold)))

    def get_accuracy(self):
        """(estimate (batch,) float64, status (batch,) uint8, flagged int) of the last factorization: status 0 solved under (B), 1 (T) below
        the threshold, 2 flagged (mode 1), 3 flagged and re-solved under (B) (mode 2); flagged = number of problems with status 2 or 3"""
        est = np.zeros(self.batch)
        st = np.zeros(self.batch, np.uint8)
        nf = C.c_uint32(0)
        capi.check(capi.lib().lexls_lse_get_accuracy(self._h, _ptr(est, C.c_double), _ptr(st, C.c_uint8), C.byref(nf)))
        return est, st, int(nf.value)
