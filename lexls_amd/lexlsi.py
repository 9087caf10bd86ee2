"""Inequality problems through the C ABI: the reference's LexLSI active-set driver (kept on the host, C++) over the
HIP equality solver.  Problem description = list of objectives, highest priority first:
  general objective        {"A": (m x n), "lb": (m,), "ub": (m,)}          lb <= A x - v <= ub
  simple bounds (first)    {"var": (m,) 0-based indices, "lb": ..., "ub": ...}
(the reference's MATLAB front end takes the same fields, interfaces/matlab-octave/lexlsi.cpp:380-445)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

PARAM_KEYS = ["max_number_of_factorizations", "tol_linear_dependence", "tol_wrong_sign_lambda", "tol_correct_sign_lambda",
              "tol_feasibility", "cycling_handling_enabled", "cycling_max_counter", "cycling_relax_step", "deactivate_first_wrong_sign"]
PARAM_DEFAULTS = [200, 1e-12, 1e-8, 1e-12, 1e-13, 0, 50, 1e-8, 0]  # typedefs.h:268-294
# the three regularization parameters of ParametersLexLSI (typedefs.h:185-187) travel only through the *_ex entry points
REG_PARAM_KEYS = ["regularization_type", "variable_regularization_factor", "max_number_of_CG_iterations"]
REG_PARAM_DEFAULTS = [0, 0.0, 10]
# the five hot-start options of ParametersLexLSI (typedefs.h:213-217), 0 / 1 each: the 17-value form of h_params
HOT_PARAM_KEYS = ["modify_x_guess_enabled", "modify_type_active_enabled", "modify_type_inactive_enabled", "set_min_init_ctr_violation", "use_phase1_v0"]
HOT_PARAM_DEFAULTS = [0, 0, 0, 1, 0]
INFO_KEYS = ["status", "iterations", "activations", "deactivations", "factorizations", "total_rank"]


class InfoRows(list):
    """the per-instance info records of a batch run: behaves like a list of dicts (status, iterations, ...), built from the (batch, 6)
    int32 array the library fills — lazily, on first access: a thousand small dicts are a third of a millisecond nobody has to pay who only
    looks at the solutions"""

    def __init__(self, array):
        super().__init__()
        self.array = array  # (batch, 6) int32, columns = INFO_KEYS
        self._built = False

    def _build(self):
        if not self._built:
            self._built = True
            super().extend(dict(zip(INFO_KEYS, row)) for row in self.array.tolist())

    def __len__(self):
        return self.array.shape[0]

    def __getitem__(self, i):
        self._build()
        return super().__getitem__(i)

    def __iter__(self):
        self._build()
        return super().__iter__()

    def __eq__(self, other):
        self._build()
        if isinstance(other, InfoRows):
            other._build()
        return list.__eq__(self, other)

    def __ne__(self, other):
        return not self.__eq__(other)

    def __repr__(self):
        self._build()
        return list.__repr__(self)


def pack_params(**kw) -> np.ndarray:
    vals = list(PARAM_DEFAULTS)
    for k, v in kw.items():
        vals[PARAM_KEYS.index(k)] = float(v)
    return np.array(vals, dtype=np.float64)


def pack_params_ex(**kw) -> np.ndarray:
    """the 9 parameters of pack_params followed by regularization_type, variable_regularization_factor, max_number_of_CG_iterations"""
    keys, vals = PARAM_KEYS + REG_PARAM_KEYS, list(PARAM_DEFAULTS) + list(REG_PARAM_DEFAULTS)
    for k, v in kw.items():
        vals[keys.index(k)] = float(v)
    return np.array(vals, dtype=np.float64)


def pack_params_hot(**kw) -> np.ndarray:
    """the 12 parameters of pack_params_ex followed by the hot-start options HOT_PARAM_KEYS"""
    keys = PARAM_KEYS + REG_PARAM_KEYS + HOT_PARAM_KEYS
    vals = list(PARAM_DEFAULTS) + list(REG_PARAM_DEFAULTS) + list(HOT_PARAM_DEFAULTS)
    for k, v in kw.items():
        vals[keys.index(k)] = float(v)
    return np.array(vals, dtype=np.float64)


def _names_hot(params) -> bool:
    return any(k in HOT_PARAM_KEYS for k in params)


def flatten(nvar: int, objectives):
    """-> dims (uint32), types (int32), data (float64, objectives back to back, column-major), var_index (uint32)"""
    dims, types, chunks, var_index = [], [], [], np.zeros(0, np.uint32)
    for k, o in enumerate(objectives):
        lb, ub = np.asarray(o["lb"], float), np.asarray(o["ub"], float)
        dims.append(lb.size)
        if "var" in o:
            if k != 0:
                raise ValueError("simple bounds are supported only in the first objective")
            types.append(1)
            var_index = np.asarray(o["var"], np.uint32)
            m = np.stack([lb, ub], axis=1)
        else:
            types.append(0)
            m = np.hstack([np.asarray(o["A"], float).reshape(lb.size, nvar), lb[:, None], ub[:, None]])
        chunks.append(np.asfortranarray(m).ravel(order="F"))
    data = np.concatenate(chunks) if chunks else np.zeros(0)
    return np.array(dims, np.uint32), np.array(types, np.int32), np.ascontiguousarray(data), np.ascontiguousarray(var_index)


def unflatten(nvar: int, dims, types, data, var_index=None):
    """inverse of flatten() for ONE problem: the flat column-major layout -> list of objective dicts"""
    objs, off = [], 0
    for d, t in zip(np.asarray(dims, int), np.asarray(types, int)):
        w = 2 if t == 1 else nvar + 2
        m = np.asarray(data[off:off + d * w], float).reshape(w, d).T  # column-major d x w
        off += d * w
        if t == 1:
            objs.append(dict(var=np.asarray(var_index, np.uint32)[:d].copy(), lb=m[:, 0].copy(), ub=m[:, 1].copy()))
        else:
            objs.append(dict(A=m[:, :nvar].copy(), lb=m[:, nvar].copy(), ub=m[:, nvar + 1].copy()))
    return objs


def _p(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def lsi_solve(nvar: int, objectives, active_guess=None, x0=None, device: int = 0, v0=None, regularization_factors=None, **params):
    """One LexLSI problem through the C ABI.  `v0`: per-objective initial residuals (list of arrays) or None; `regularization_factors`:
    one per objective or None; `params`: ParametersLexLSI fields (PARAM_KEYS + REG_PARAM_KEYS)."""
    dims, types, data, var_index = flatten(nvar, objectives)
    total = int(dims.sum())
    x, info = np.zeros(nvar), np.zeros(6, np.int32)
    active, v = np.zeros(total, np.uint8), np.zeros(total)
    guess = None if active_guess is None else np.ascontiguousarray(np.concatenate([np.asarray(g, np.uint8) for g in active_guess]))
    x0a = None if x0 is None else np.ascontiguousarray(x0, np.float64)
    extended = v0 is not None or regularization_factors is not None or any(k in REG_PARAM_KEYS for k in params) or _names_hot(params)
    if extended:
        v0a = None if v0 is None else np.ascontiguousarray(np.concatenate([np.asarray(a, np.float64) for a in v0]))
        rfa = None if regularization_factors is None else np.ascontiguousarray(regularization_factors, np.float64)
        par = pack_params_hot(**params) if _names_hot(params) else pack_params_ex(**params)
        capi.check(capi.lib().lexls_lsi_solve_ex(
            C.c_int(device), C.c_uint32(nvar), C.c_uint32(len(dims)), _p(dims, C.c_uint32), _p(types, C.c_int32), _p(data, C.c_double),
            _p(var_index if var_index.size else None, C.c_uint32), _p(guess, C.c_uint8), _p(x0a, C.c_double), _p(v0a, C.c_double),
            _p(rfa, C.c_double), _p(par, C.c_double), C.c_uint32(len(par)), _p(x, C.c_double), _p(info, C.c_int32), _p(active, C.c_uint8),
            _p(v, C.c_double)))
    else:
        par = pack_params(**params)
        capi.check(capi.lib().lexls_lsi_solve(
            C.c_int(device), C.c_uint32(nvar), C.c_uint32(len(dims)), _p(dims, C.c_uint32), _p(types, C.c_int32), _p(data, C.c_double),
            _p(var_index if var_index.size else None, C.c_uint32), _p(guess, C.c_uint8), _p(x0a, C.c_double), _p(par, C.c_double),
            _p(x, C.c_double), _p(info, C.c_int32), _p(active, C.c_uint8), _p(v, C.c_double)))
    cuts = np.cumsum(dims)[:-1]
    return dict(x=x, info=dict(zip(INFO_KEYS, info.tolist())), active=np.split(active, cuts), v=np.split(v, cuts))


class _DebugStruct(C.Structure):
    """lexls_lsi_debug of include/lexls_hip.h"""
    _fields_ = [("lambda_", C.c_void_p), ("lexqr", C.c_void_p), ("data", C.c_void_p), ("x_star", C.c_void_p), ("active_ctr", C.c_void_p),
                ("log", C.c_void_p), ("log_alpha", C.c_void_p), ("max_log", C.c_uint32), ("x_mu", C.c_void_p), ("x_mu_rhs", C.c_void_p),
                ("residual_mu", C.c_void_p), ("counts", C.c_void_p)]


def debug_buffers(nvar: int, dims, max_log: int = 4096):
    """numpy arrays for the debug outputs of one LexLSI solve (lexls_lsi_debug); shaped into the MEX structure by debug_structure()"""
    total, nobj = int(np.sum(dims)), len(dims)
    return dict(lam=np.zeros((nobj, total)), lexqr=np.zeros((nvar + 1, total)), data=np.zeros((nvar + 1, total)), x_star=np.zeros(nvar),
                active_ctr=np.zeros((total, 3), np.int32), log=np.zeros((max_log, 5), np.int32), log_alpha=np.zeros(max_log),
                x_mu=np.zeros((nobj, nvar)), x_mu_rhs=np.zeros((nobj, nvar)), residual_mu=np.zeros(total), counts=np.zeros(4, np.uint32))


def debug_structure(nvar: int, dims, buf, with_mu: bool):
    """the fields of formDebugStructure (interfaces/matlab-octave/lexlsi.cpp:77-260) from filled debug_buffers()"""
    rows, nobjl, nact, nlog = (int(c) for c in buf["counts"])
    cuts = np.cumsum(dims)[:-1]
    nlog = min(nlog, buf["log"].shape[0])
    d = {
        "working_set_log": [dict(obj_index=int(e[0]), ctr_index=int(e[1]), ctr_type=int(e[2]), alpha_or_lambda=float(a), cycling_detected=int(e[3]), rank=int(e[4]))
                            for e, a in zip(buf["log"][:nlog], buf["log_alpha"][:nlog])],
        "active_ctr": [dict(obj_index=int(e[0]), ctr_index=int(e[1]), ctr_type=int(e[2])) for e in buf["active_ctr"][:nact]],
        "lambda": np.split(np.ascontiguousarray(buf["lam"].T), cuts),  # one (dim_k x nObj) matrix per objective
        "lexqr": np.ascontiguousarray(buf["lexqr"].reshape(-1)[:rows * (nvar + 1)].reshape(nvar + 1, rows).T),
        "data": np.ascontiguousarray(buf["data"].reshape(-1)[:rows * (nvar + 1)].reshape(nvar + 1, rows).T),
        "xStar": buf["x_star"],
    }
    if with_mu:
        d.update(X_mu=np.ascontiguousarray(buf["x_mu"][:nobjl].T), X_mu_rhs=np.ascontiguousarray(buf["x_mu_rhs"][:nobjl].T), residual_mu=buf["residual_mu"][:rows])
    return d


def lsi_solve_debug(nvar: int, objectives, active_guess=None, x0=None, device: int = 0, v0=None, regularization_factors=None, max_log: int = 4096, **params):
    """lsi_solve plus the MEX front end's debug structure `d` (lexls_lsi_solve_debug): returns the lsi_solve dict with key "debug"."""
    dims, types, data, var_index = flatten(nvar, objectives)
    total = int(dims.sum())
    x, info = np.zeros(nvar), np.zeros(6, np.int32)
    active, v = np.zeros(total, np.uint8), np.zeros(total)
    guess = None if active_guess is None else np.ascontiguousarray(np.concatenate([np.asarray(g, np.uint8) for g in active_guess]))
    x0a = None if x0 is None else np.ascontiguousarray(x0, np.float64)
    v0a = None if v0 is None else np.ascontiguousarray(np.concatenate([np.asarray(a, np.float64) for a in v0]))
    rfa = None if regularization_factors is None else np.ascontiguousarray(regularization_factors, np.float64)
    par = pack_params_hot(**params) if _names_hot(params) else pack_params_ex(**params)
    buf = debug_buffers(nvar, dims, max_log)
    ds = _DebugStruct(buf["lam"].ctypes.data, buf["lexqr"].ctypes.data, buf["data"].ctypes.data, buf["x_star"].ctypes.data, buf["active_ctr"].ctypes.data,
                      buf["log"].ctypes.data, buf["log_alpha"].ctypes.data, max_log, buf["x_mu"].ctypes.data, buf["x_mu_rhs"].ctypes.data,
                      buf["residual_mu"].ctypes.data, buf["counts"].ctypes.data)
    capi.check(capi.lib().lexls_lsi_solve_debug(
        C.c_int(device), C.c_uint32(nvar), C.c_uint32(len(dims)), _p(dims, C.c_uint32), _p(types, C.c_int32), _p(data, C.c_double),
        _p(var_index if var_index.size else None, C.c_uint32), _p(guess, C.c_uint8), _p(x0a, C.c_double), _p(v0a, C.c_double),
        _p(rfa, C.c_double), _p(par, C.c_double), C.c_uint32(len(par)), _p(x, C.c_double), _p(info, C.c_int32), _p(active, C.c_uint8),
        _p(v, C.c_double), C.byref(ds)))
    cuts = np.cumsum(dims)[:-1]
    return dict(x=x, info=dict(zip(INFO_KEYS, info.tolist())), active=np.split(active, cuts), v=np.split(v, cuts),
                debug=debug_structure(nvar, dims, buf, int(params.get("regularization_type", 0)) == 7))


def lsi_solve_dat(path: str, nvar: int, one_based=True, use_active_guess=False, use_x_guess=False, device: int = 0):
    x, sol, info = np.zeros(nvar), np.zeros(nvar), np.zeros(6, np.int32)
    capi.check(capi.lib().lexls_lsi_solve_dat(C.c_int(device), path.encode(), C.c_int(one_based), C.c_int(use_active_guess), C.c_int(use_x_guess),
                                              _p(x, C.c_double), _p(info, C.c_int32), _p(sol, C.c_double)))
    return dict(x=x, solution=sol, info=dict(zip(INFO_KEYS, info.tolist())))


class PackedBatch:
    """A batch of same-structure LexLSI problems in the flat layout lexls_lsi_batch_solve takes (include/lexls_hip.h): build it once
    with pack_batch() when the same constraint data is solved repeatedly (warm starts) — flattening Python objective lists costs far
    more than the solve."""

    def __init__(self, nvar, dims, types, data, var_index):
        self.nvar, self.dims, self.types, self.data, self.var_index = nvar, dims, types, data, var_index
        self.batch, self.total = data.shape[0], int(dims.sum())


def pack_batch(nvar: int, problems) -> PackedBatch:
    flat = [flatten(nvar, objs) for objs in problems]
    dims, types = flat[0][0], flat[0][1]
    for f in flat:
        if not (np.array_equal(f[0], dims) and np.array_equal(f[1], types)):
            raise ValueError("all problems of a batch must share dims and objective types")
    data = np.ascontiguousarray(np.stack([f[2] for f in flat]))
    var_index = np.ascontiguousarray(np.stack([f[3] for f in flat])) if flat[0][3].size else None
    return PackedBatch(nvar, dims, types, data, var_index)


class LsiBatch:
    """A lock-step batch that outlives one solve (lexls_lsi_batch_create / _run / _destroy): device buffers, pinned blocks, streams and the
    host worker pool are made once for `batch` problems of one structure; every run() solves new data of that structure."""

    def __init__(self, nvar: int, dims, types, batch: int, device: int = 0):
        self.nvar, self.batch, self.device = int(nvar), int(batch), int(device)
        self.dims = np.ascontiguousarray(dims, np.uint32)
        self.types = np.ascontiguousarray(types, np.int32)
        self.total = int(self.dims.sum())
        self._h = C.c_void_p()
        self._run_serial = 0  # counts the runs started on this batch (run / run_device / enqueue_device): what a backward pass checks its forward run by
        self._log_entries = 0  # capacity per instance of the working-set log (set_working_set_log); 0: off
        self._instance_factors = None  # the device tensor (or address) set_instance_regularization was given: kept alive while the library reads it
        self._instance_mask = None  # the device tensor set_instance_mask was given: kept alive while the library reads it
        self._instance_limits = None  # the device tensor set_instance_max_factorizations was given: kept alive while the library reads it
        self._instance_obj_dims = None  # the device tensor set_instance_obj_dims was given: kept alive while the library reads it
        capi.check(capi.lib().lexls_lsi_batch_create(C.byref(self._h), C.c_int(device), C.c_uint32(self.batch), C.c_uint32(self.nvar),
                                                     C.c_uint32(len(self.dims)), _p(self.dims, C.c_uint32), _p(self.types, C.c_int32)))

    def close(self):
        if self._h:
            capi.lib().lexls_lsi_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self) -> dict:
        """of the last run: stage counts and whether the iteration step ran on the device (LEXLS_LSI_DEVICE_STEP=1 at creation)"""
        st = np.zeros(4, np.int32)
        capi.check(capi.lib().lexls_lsi_batch_stats(self._h, _p(st, C.c_int32)))
        return dict(factorize_solve=int(st[0]), sensitivity=int(st[1]), device_step=int(st[2]), groups=int(st[3]))

    def final_factorizations(self) -> int:
        """lexls_lsi_batch_final_factorizations: how often, since creation, a group's final equality problems were formed and factorized — the
        stage lambdas(), solve_adjoint*() and solve_adjoint_matrix*() share (once per run and group, whichever call comes first)"""
        count = C.c_uint32(0)
        capi.check(capi.lib().lexls_lsi_batch_final_factorizations(self._h, C.byref(count)))
        return int(count.value)

    def last_kernel(self) -> str:
        """the kernel that served the resident active-set iterations of the last run (lexls_lsi_batch_last_kernel): the persistent launch
        ("lsi_fused<...>", with "regularized" for a regularized run), the l-QR kernel of the lock-step stages, or "host" when the run was not
        resident (LEXLS_LSI_RESIDENT=0, regularization type 7, cycling handling of a regularized run, ...)"""
        return capi.lib().lexls_lsi_batch_last_kernel(self._h).decode()

    def set_instance_regularization(self, factors):
        """lexls_lsi_batch_set_instance_regularization: regularization factors of its own for every instance, (batch, nObj), in place of the
        shared `regularization_factors=` of run() / run_device() — which then must not be given (the library's error is raised).  A numpy array
        (or anything array-like) is copied at the call; a torch tensor on the batch's device (float64, contiguous) or an integer device address
        is KEPT and read at the start of every run, so it may be rewritten in place between runs — the caller keeps it alive.  None clears
        the setting.  A run with regularization_type 0 ignores it."""
        nobj, keep = len(self.dims), None
        if factors is None:
            ptr, on_device = None, 0
        elif hasattr(factors, "data_ptr"):
            import torch
            ptr, on_device, keep = self._device_array("factors", factors, torch.float64, (self.batch, nobj), optional=False), 1, factors
        elif isinstance(factors, int):
            ptr, on_device, keep = C.c_void_p(factors), 1, factors
        else:
            f = np.ascontiguousarray(factors, np.float64)
            if f.shape != (self.batch, nobj):
                raise ValueError(f"set_instance_regularization: factors have shape {f.shape}, {(self.batch, nobj)} expected")
            ptr, on_device = C.c_void_p(f.ctypes.data), 0
        capi.check(capi.lib().lexls_lsi_batch_set_instance_regularization(self._h, ptr, C.c_int(on_device)))
        self._instance_factors = keep  # (a tensor given earlier is let go of only now that the library has another source)

    def set_instance_mask(self, mask):
        """lexls_lsi_batch_set_instance_mask: `mask` is a torch uint8 or bool tensor of `batch` elements on the batch's device (contiguous), or None to
        clear the setting.  An instance whose byte is 0 is skipped by every later run_device() / enqueue_device(): nothing of its inputs is read and
        its rows of the caller's outputs keep their bits (run_device() makes new, zeroed tensors: pass the previous ones through enqueue_device's
        `out` to keep answers); the host's view of the run shows it as an empty entry.  The tensor is KEPT — a reference is held so the memory stays
        alive — and read on the device at the start of every run, so it may be rewritten in place between runs and between replays of a captured
        enqueue_device().  While a mask is set, run() raises (LEXLS_ERR_UNSUPPORTED)."""
        if mask is None:
            ptr = None
        else:
            import torch
            if not hasattr(mask, "data_ptr") or mask.dtype not in (torch.uint8, torch.bool):
                raise TypeError("set_instance_mask: mask must be a torch uint8 or bool tensor on the batch's device, or None")
            ptr = self._device_array("mask", mask, mask.dtype, (self.batch,), optional=False)
        capi.check(capi.lib().lexls_lsi_batch_set_instance_mask(self._h, ptr))
        self._instance_mask = mask  # (a tensor given earlier is let go of only now that the library has another source)

    def set_instance_max_factorizations(self, limits):
        """lexls_lsi_batch_set_instance_max_factorizations: `limits` is a torch int32 tensor of shape (batch,) on the batch's device (contiguous), or
        None to clear the setting.  In every later run_device() / enqueue_device() an instance whose entry L is >= 1 runs as one LexLSI object with
        max_number_of_factorizations = min(L, the run's parameter); an entry <= 0 leaves it the run's parameter.  The tensor is KEPT — a reference is
        held so the memory stays alive — and read on the device at the start of every run, so it may be rewritten in place between runs and between
        replays of a captured enqueue_device(); a run in flight keeps the values it started with.  While limits are set, run() raises
        (LEXLS_ERR_UNSUPPORTED)."""
        if limits is None:
            ptr = None
        else:
            import torch
            if not hasattr(limits, "data_ptr") or limits.dtype != torch.int32:
                raise TypeError("set_instance_max_factorizations: limits must be a torch int32 tensor on the batch's device, or None")
            ptr = self._device_array("limits", limits, torch.int32, (self.batch,), optional=False)
        capi.check(capi.lib().lexls_lsi_batch_set_instance_max_factorizations(self._h, ptr))
        self._instance_limits = limits  # (a tensor given earlier is let go of only now that the library has another source)

    def set_instance_obj_dims(self, dims):
        """lexls_lsi_batch_set_instance_obj_dims: `dims` is a torch uint32 or int32 tensor of shape (batch, nObj) on the batch's device (contiguous), or
        None to clear the setting.  In every later run_device() / enqueue_device() objective k of instance i consists of the first dims[i, k] rows of
        its block; the batch's own dims are the capacities and stay the layout of every array (data, var_index, active_guess, v0 and the outputs).
        Rows beyond an instance's count are absent: nothing of them is read, their rows of active / v / lambda are written as 0.  A count above its
        capacity is an input error of the run (code 5), 0 is an empty objective.  The tensor is KEPT — a reference is held so the memory stays alive —
        and read on the device at the start of every run, so it may be rewritten in place between runs and between replays of a captured
        enqueue_device(); a run in flight keeps the values it started with.  While counts are set, run() raises (LEXLS_ERR_UNSUPPORTED)."""
        if dims is None:
            ptr = None
        else:
            import torch
            if not hasattr(dims, "data_ptr") or dims.dtype not in (torch.uint32, torch.int32):
                raise TypeError("set_instance_obj_dims: dims must be a torch uint32 or int32 tensor on the batch's device, or None")
            if tuple(dims.shape) != (self.batch, len(self.dims)):
                raise ValueError(f"set_instance_obj_dims: dims have shape {tuple(dims.shape)}, {(self.batch, len(self.dims))} expected")
            ptr = self._device_array("dims", dims, dims.dtype, (self.batch, len(self.dims)), optional=False)
        capi.check(capi.lib().lexls_lsi_batch_set_instance_obj_dims(self._h, ptr))
        self._instance_obj_dims = dims  # (a tensor given earlier is let go of only now that the library has another source)

    def run(self, problems, active_guess=None, x0=None, regularization_factors=None, v0=None, **params):
        """`problems`: list of objective lists or a PackedBatch of this batch's structure; other arguments as lsi_batch_solve"""
        pk = problems if isinstance(problems, PackedBatch) else pack_batch(self.nvar, problems)
        if pk.batch != self.batch or not np.array_equal(pk.dims, self.dims) or not np.array_equal(pk.types, self.types):
            raise ValueError("problems do not have the structure this batch was created for")
        batch, total, nvar = self.batch, self.total, self.nvar
        guess = None
        if isinstance(active_guess, np.ndarray):
            guess = np.ascontiguousarray(active_guess.reshape(batch, total), np.uint8)
        elif active_guess is not None:
            guess = np.ascontiguousarray(np.stack([np.concatenate([np.asarray(g, np.uint8) for g in ag]) for ag in active_guess]))
        x0a = None if x0 is None else np.ascontiguousarray(x0, np.float64)
        v0a = None if v0 is None else np.ascontiguousarray(np.asarray(v0, np.float64).reshape(batch, total))  # initial residuals, (batch, sum(dims))
        x, info = np.zeros((batch, nvar)), np.zeros((batch, 6), np.int32)
        active, v, rounds = np.zeros((batch, total), np.uint8), np.zeros((batch, total)), np.zeros(2, np.int32)
        if _names_hot(params):
            par = pack_params_hot(**params)
        elif regularization_factors is not None or any(k in REG_PARAM_KEYS for k in params):
            par = pack_params_ex(**params)
        else:
            par = pack_params(**params)
        rfa = None if regularization_factors is None else np.ascontiguousarray(regularization_factors, np.float64)
        if hasattr(self._instance_factors, "data_ptr"):
            import torch
            torch.cuda.synchronize(torch.device("cuda", self.device))  # what wrote the factor tensor is complete before the library's streams read it
        self._run_serial += 1
        capi.check(capi.lib().lexls_lsi_batch_run(
            self._h, _p(pk.data, C.c_double), _p(pk.var_index, C.c_uint32), _p(guess, C.c_uint8), _p(x0a, C.c_double), _p(v0a, C.c_double), _p(rfa, C.c_double),
            _p(par, C.c_double), C.c_uint32(len(par)), _p(x, C.c_double), _p(info, C.c_int32), _p(active, C.c_uint8), _p(v, C.c_double),
            _p(rounds, C.c_int32)))
        return dict(x=x, info=InfoRows(info), active=active, v=v,
                    rounds=dict(factorize_solve=int(rounds[0]), sensitivity=int(rounds[1])), dims=self.dims)

    def _device_array(self, name, t, dtype, shape, optional=True):
        """the device address of a caller's tensor (anything with data_ptr(), i.e. torch tensors) after checking what the library takes for granted"""
        if t is None:
            if optional:
                return None
            raise ValueError(f"run_device: {name} is required")
        if not hasattr(t, "data_ptr"):
            raise TypeError(f"run_device: {name} must be a device tensor (something with data_ptr()), not {type(t).__name__}")
        import torch
        if t.dtype != dtype:
            raise TypeError(f"run_device: {name} must be {dtype}, not {t.dtype}")
        if t.device.type != "cuda" or (t.device.index or 0) != self.device:
            raise ValueError(f"run_device: {name} is on {t.device}, the batch is on device {self.device}")
        if not t.is_contiguous():
            raise ValueError(f"run_device: {name} must be contiguous")
        if t.numel() != int(np.prod(shape)):
            raise ValueError(f"run_device: {name} has {t.numel()} elements, {tuple(shape)} expected")
        return C.c_void_p(t.data_ptr())

    def run_device(self, data, var_index=None, active_guess=None, x0=None, regularization_factors=None, v0=None, with_lambda=False,
                   with_cycling_counters=False, **params):
        """lexls_lsi_batch_run_device: a run whose problems are on the batch's device already and whose results stay there.  `data`: float64
        (batch, per-instance data) in the flat layout of PackedBatch.data; `var_index`: int32 (batch, dims[0]), required when objective 0 holds
        simple bounds; `active_guess`: uint8 (batch, total) or None; `x0`: float64 (batch, nvar) or None — torch tensors (anything with
        data_ptr()), contiguous.  Returns {"x", "info", "active", "v"} as torch tensors on that device (info: (batch, 6) int32, columns
        INFO_KEYS).  Only runs that are resident on the device are served; everything else raises (LEXLS_ERR_UNSUPPORTED), nothing is computed
        on the host instead.  stats(), last_kernel(), lambdas() and cycling_counters() work afterwards as after run().

        The rest of a warm start and of the results on the device (lexls_lsi_batch_run_device_ex; without these keywords the call above is made):
        `v0`: float64 (batch, total) initial residuals, taken as they stand together with x0 and disregarded without it (the reference's set_v0);
        `with_lambda`: the result also has "lambda", (batch, nObj, total) float64, the layout of lambda_array() — raises (LEXLS_ERR_UNSUPPORTED,
        nothing computed) for a run with cycling handling or regularization; `with_cycling_counters`: the result also has "cycling_counters",
        (batch,) int32 holding the uint32 bits of cycling_counters()."""
        import torch
        batch, total, nvar = self.batch, self.total, self.nvar
        per_data = int(sum(int(d) * (2 if t == 1 else nvar + 2) for d, t in zip(self.dims, self.types)))
        simple = int(self.types[0]) == 1
        d_data = self._device_array("data", data, torch.float64, (batch, per_data), optional=False)
        d_var = self._device_array("var_index", var_index, torch.int32, (batch, int(self.dims[0])), optional=not simple) if simple else None
        d_guess = self._device_array("active_guess", active_guess, torch.uint8, (batch, total))
        d_x0 = self._device_array("x0", x0, torch.float64, (batch, nvar))
        d_v0 = self._device_array("v0", v0, torch.float64, (batch, total))
        if _names_hot(params):
            par = pack_params_hot(**params)
        elif regularization_factors is not None or any(k in REG_PARAM_KEYS for k in params):
            par = pack_params_ex(**params)
        else:
            par = pack_params(**params)
        rfa = None if regularization_factors is None else np.ascontiguousarray(regularization_factors, np.float64)
        dev = torch.device("cuda", self.device)
        x = torch.zeros((batch, nvar), dtype=torch.float64, device=dev)
        info = torch.zeros((batch, 6), dtype=torch.int32, device=dev)
        active = torch.zeros((batch, total), dtype=torch.uint8, device=dev)
        v = torch.zeros((batch, total), dtype=torch.float64, device=dev)
        r = dict(x=x, info=info, active=active, v=v)
        if with_lambda:
            r["lambda"] = torch.zeros((batch, len(self.dims), total), dtype=torch.float64, device=dev)
        if with_cycling_counters:
            r["cycling_counters"] = torch.zeros((batch,), dtype=torch.int32, device=dev)
        self._run_serial += 1
        torch.cuda.synchronize(dev)  # the inputs (and the zeroed outputs) are complete before the library's own streams read and write them
        out = [C.c_void_p(x.data_ptr()), C.c_void_p(info.data_ptr()), C.c_void_p(active.data_ptr()), C.c_void_p(v.data_ptr())]
        if v0 is None and not with_lambda and not with_cycling_counters:
            capi.check(capi.lib().lexls_lsi_batch_run_device(
                self._h, d_data, d_var, d_guess, d_x0, _p(rfa, C.c_double), _p(par, C.c_double), C.c_uint32(len(par)), *out))
        else:
            capi.check(capi.lib().lexls_lsi_batch_run_device_ex(
                self._h, d_data, d_var, d_guess, d_x0, d_v0, _p(rfa, C.c_double), _p(par, C.c_double), C.c_uint32(len(par)), *out,
                C.c_void_p(r["lambda"].data_ptr()) if with_lambda else None,
                C.c_void_p(r["cycling_counters"].data_ptr()) if with_cycling_counters else None))
        return r

    def enqueue_device(self, data, var_index=None, active_guess=None, x0=None, regularization_factors=None, v0=None, with_lambda=False,
                       with_cycling_counters=False, stream=None, status=None, out=None, **params):
        """lexls_lsi_batch_enqueue_device: run_device() as work in a stream — the same tensors, keywords and results, but the call only enqueues
        the run and returns; nothing is waited for, so the inputs need only be complete in stream order and the returned tensors are complete
        for work enqueued later in the same stream.  `stream`: a torch.cuda.Stream or a raw hipStream_t address; None: torch's current stream.
        `status`: an int32 tensor of one element on the device, or None — it receives -1 (0xffffffff) for a good run and instance * 8 + code for
        a run with an input error, whose other outputs are left as they were.  `out`: {"x", "info", "active", "v"[, "cycling_counters"]} to
        write into (shapes and dtypes of run_device's result) instead of new tensors.  The host's view of the run — stats(), last_kernel(),
        lambdas(), cycling_counters(), the working-set log — is there after finish(); until then those calls raise.  Only runs whose resident
        iterations are one persistent launch are served (LEXLS_ERR_UNSUPPORTED otherwise, nothing enqueued; so for a batch that LEXLS_LSI_GROUPS
        splits into groups).  The call may be captured (torch.cuda.graph) once the batch has served one uncaptured
        enqueue_device() + finish() with the same options; while the graph is in use, finish() is the only other call on the batch."""
        import torch
        batch, total, nvar = self.batch, self.total, self.nvar
        per_data = int(sum(int(d) * (2 if t == 1 else nvar + 2) for d, t in zip(self.dims, self.types)))
        simple = int(self.types[0]) == 1
        d_data = self._device_array("data", data, torch.float64, (batch, per_data), optional=False)
        d_var = self._device_array("var_index", var_index, torch.int32, (batch, int(self.dims[0])), optional=not simple) if simple else None
        d_guess = self._device_array("active_guess", active_guess, torch.uint8, (batch, total))
        d_x0 = self._device_array("x0", x0, torch.float64, (batch, nvar))
        d_v0 = self._device_array("v0", v0, torch.float64, (batch, total))
        d_status = self._device_array("status", status, torch.int32, (1,))
        if _names_hot(params):
            par = pack_params_hot(**params)
        elif regularization_factors is not None or any(k in REG_PARAM_KEYS for k in params):
            par = pack_params_ex(**params)
        else:
            par = pack_params(**params)
        rfa = None if regularization_factors is None else np.ascontiguousarray(regularization_factors, np.float64)
        dev = torch.device("cuda", self.device)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        shapes = dict(x=((batch, nvar), torch.float64), info=((batch, 6), torch.int32), active=((batch, total), torch.uint8), v=((batch, total), torch.float64))
        if with_lambda:
            shapes["lambda"] = ((batch, len(self.dims), total), torch.float64)
        if with_cycling_counters:
            shapes["cycling_counters"] = ((batch,), torch.int32)
        r = {}
        for k, (shape, dtype) in shapes.items():
            if out is not None and k in out:
                self._device_array(k, out[k], dtype, shape, optional=False)
                r[k] = out[k]
            elif isinstance(stream, torch.cuda.Stream):
                with torch.cuda.stream(stream):  # the fill is ordered in front of the run
                    r[k] = torch.zeros(shape, dtype=dtype, device=dev)
            else:
                r[k] = torch.empty(shape, dtype=dtype, device=dev)  # (a raw stream: torch cannot order a fill in it; a good run writes every element)
        self._run_serial += 1
        handle = stream.cuda_stream if isinstance(stream, torch.cuda.Stream) else int(stream)
        capi.check(capi.lib().lexls_lsi_batch_enqueue_device(
            self._h, C.c_void_p(handle), d_data, d_var, d_guess, d_x0, d_v0, _p(rfa, C.c_double), _p(par, C.c_double), C.c_uint32(len(par)),
            *(C.c_void_p(r[k].data_ptr()) for k in ("x", "info", "active", "v")),
            C.c_void_p(r["lambda"].data_ptr()) if with_lambda else None,
            C.c_void_p(r["cycling_counters"].data_ptr()) if with_cycling_counters else None, d_status))
        return r

    def finish(self, stream=None):
        """lexls_lsi_batch_finish: waits for `stream` (a torch.cuda.Stream or a raw address; None: the stream of the last enqueue_device()) and
        fetches what stats(), last_kernel(), lambdas(), cycling_counters() and the working-set log answer from.  Raises (LEXLS_ERR_INVALID, the
        instance and the reason in the message) when the run had an input error; the batch then takes the next run normally.  After a replay
        of a captured enqueue_device(), finish(replay_stream) answers for that replay."""
        handle = None if stream is None else C.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))
        capi.check(capi.lib().lexls_lsi_batch_finish(self._h, handle))

    def cycling_counters(self) -> np.ndarray:
        """LexLSI::getCyclingCounter() of every instance of the last run (lexls_lsi_batch_get_cycling_counters): (batch,) uint32, the bounds each
        instance's cycling handler relaxed; zeros after a run without cycling_handling_enabled"""
        counts = np.zeros(self.batch, np.uint32)
        capi.check(capi.lib().lexls_lsi_batch_get_cycling_counters(self._h, _p(counts, C.c_uint32)))
        return counts

    def set_adjoint_regularized(self, on: bool = True):
        """lexls_lsi_batch_set_adjoint_regularized: from the next run on, solve_adjoint / solve_adjoint_device also answer after a regularized run
        that was resident on the device, of regularization type 1, 3, 4, 5, 8 or 9 with variable_regularization_factor == 0: the gradient of the
        damped final equality problem, the factors (shared or per instance) held fixed as the matrices are.  Off by default: every regularized
        run is refused, as before.  lambdas() and solve_adjoint_matrix refuse regularized runs either way; solve_adjoint_multi has a switch of its
        own (set_adjoint_regularized_multi)."""
        capi.check(capi.lib().lexls_lsi_batch_set_adjoint_regularized(self._h, C.c_int(1 if on else 0)))
        self._adj_reg = bool(on)

    def set_adjoint_regularized_multi(self, on: bool = True):
        """lexls_lsi_batch_set_adjoint_regularized_multi: from the next run on, solve_adjoint_multi / solve_adjoint_multi_device (and
        jacobian_bounds_device) also answer after a regularized run, under the conditions of set_adjoint_regularized().  Off by default and
        independent of that switch; the damped final factor is built once per run and shared by both calls."""
        capi.check(capi.lib().lexls_lsi_batch_set_adjoint_regularized_multi(self._h, C.c_int(1 if on else 0)))
        self._adj_reg_multi = bool(on)

    def _one_cotangent_on_the_multi_entry(self):
        """K == 1 goes to solve_adjoint — unless the batch switched the damped adjoint on for the multi calls alone (solve_adjoint would refuse a
        regularized run then)"""
        return getattr(self, "_adj_reg_multi", False) and not getattr(self, "_adj_reg", False)

    def set_working_set_log(self, max_entries: int):
        """lexls_lsi_batch_set_working_set_log: every later run() / run_device() keeps the working-set log of each instance
        (LexLSI::getWorkingSetLog), up to `max_entries` entries per instance; 0 switches the log off again and frees its buffers"""
        max_entries = int(max_entries)
        if max_entries < 0:
            raise ValueError("set_working_set_log: max_entries must not be negative")
        capi.check(capi.lib().lexls_lsi_batch_set_working_set_log(self._h, C.c_uint32(max_entries)))
        self._log_entries = max_entries

    def working_set_log_arrays(self):
        """the raw arrays of lexls_lsi_batch_get_working_set_log for the last run: log (batch, max_entries, 5) int32 with the columns
        capi.WORKING_SET_LOG_FIELDS, alpha_or_lambda (batch, max_entries) float64, counts (batch,) uint32 — the entries each instance produced,
        which may exceed max_entries (the rest was dropped)"""
        cap = self._log_entries
        log = np.zeros((self.batch, cap, len(capi.WORKING_SET_LOG_FIELDS)), np.int32)
        alpha, counts = np.zeros((self.batch, cap)), np.zeros(self.batch, np.uint32)
        capi.check(capi.lib().lexls_lsi_batch_get_working_set_log(self._h, _p(log, C.c_int32), _p(alpha, C.c_double), _p(counts, C.c_uint32)))
        return log, alpha, counts

    def working_set_log(self):
        """-> (logs, counts): per instance of the last run the list of entries that frontend.lexlsi(..., debug=True) returns as
        d["working_set_log"] (dicts with obj_index, ctr_index, ctr_type, alpha_or_lambda, cycling_detected, rank), cut at max_entries, and the
        (batch,) uint32 number of entries each instance produced"""
        log, alpha, counts = self.working_set_log_arrays()
        logs = [[dict(alpha_or_lambda=float(a), **{k: int(f) for k, f in zip(capi.WORKING_SET_LOG_FIELDS, e)}) for e, a in zip(log[b][:int(c)], alpha[b][:int(c)])]
                for b, c in enumerate(counts)]
        return logs, counts

    def working_set_log_device(self):
        """lexls_lsi_batch_working_set_log_device: {"log", "alpha_or_lambda", "counts"} as torch tensors over the library's own device arrays — no
        copy; (batch, max_entries, 5) int32, (batch, max_entries) float64, (batch,) int32 holding the uint32 bits of the counts.  They describe
        the last run once run() / run_device() has returned and are valid until the next set_working_set_log() or close()."""
        import torch
        ptr = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        capi.check(capi.lib().lexls_lsi_batch_working_set_log_device(self._h, *(C.byref(p) for p in ptr)))
        cap, dev = self._log_entries, torch.device("cuda", self.device)

        class _Span:  # the CUDA array interface over memory this object does not own
            def __init__(self, address, shape, typestr):
                self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(int(address), False), version=2, strides=None)

        shapes = [((self.batch, cap, len(capi.WORKING_SET_LOG_FIELDS)), "<i4"), ((self.batch, cap), "<f8"), ((self.batch,), "<i4")]
        return {k: torch.as_tensor(_Span(p.value, s, t), device=dev) for k, p, (s, t) in zip(("log", "alpha_or_lambda", "counts"), ptr, shapes)}

    def lambda_array(self) -> np.ndarray:
        """getLambda of every instance of the last run (lexls_lsi_batch_get_lambda): (batch, nObj, total) — instance b's total x nObj
        column-major matrix, row = constraint in the user's order (objectives stacked), column = objective"""
        lam = np.zeros((self.batch, len(self.dims), self.total))
        capi.check(capi.lib().lexls_lsi_batch_get_lambda(self._h, _p(lam, C.c_double)))
        return lam

    def solve_adjoint(self, g):
        """lexls_lsi_batch_solve_adjoint: `g` = dloss/dx of the last run, (batch, nvar).  Returns (grad_lb, grad_ub), numpy arrays of shape
        (batch, total) in the constraint order of `active` / `v`: dloss/dlb and dloss/dub with the matrices held fixed.  An active constraint's
        value is in grad_lb (active at its lower bound) or grad_ub (upper bound, equality); everything outside the final working set, and every
        row of an instance that did not end PROBLEM_SOLVED, is exactly 0.  Raises after the runs lambdas() raises after — except, once
        set_adjoint_regularized() is on, after a resident regularized run of type 1, 3, 4, 5, 8 or 9 with constant factors: then the gradient is
        that of the damped final problem, the factors held fixed."""
        g = np.ascontiguousarray(g, np.float64)
        if g.shape != (self.batch, self.nvar):
            raise ValueError(f"solve_adjoint: g has shape {g.shape}, {(self.batch, self.nvar)} expected")
        grad_lb, grad_ub = np.zeros((self.batch, self.total)), np.zeros((self.batch, self.total))
        capi.check(capi.lib().lexls_lsi_batch_solve_adjoint(self._h, _p(g, C.c_double), _p(grad_lb, C.c_double), _p(grad_ub, C.c_double)))
        return grad_lb, grad_ub

    def solve_adjoint_device(self, g, grad_lb=None, grad_ub=None):
        """lexls_lsi_batch_solve_adjoint_device: solve_adjoint() on torch tensors of the batch's device — `g` float64 (batch, nvar), `grad_lb` and
        `grad_ub` float64 (batch, total), contiguous; an output that is not given is allocated (zeroed).  Returns (grad_lb, grad_ub).  Nothing of
        them passes through host memory.  Under an instance mask the rows of a skipped instance keep their bits: pass the tensors that hold
        them.  The call waits for the device, like run_device()."""
        import torch
        d_g = self._device_array("g", g, torch.float64, (self.batch, self.nvar), optional=False)
        dev = torch.device("cuda", self.device)
        if grad_lb is None:
            grad_lb = torch.zeros((self.batch, self.total), dtype=torch.float64, device=dev)
        if grad_ub is None:
            grad_ub = torch.zeros((self.batch, self.total), dtype=torch.float64, device=dev)
        d_lb = self._device_array("grad_lb", grad_lb, torch.float64, (self.batch, self.total), optional=False)
        d_ub = self._device_array("grad_ub", grad_ub, torch.float64, (self.batch, self.total), optional=False)
        torch.cuda.synchronize(dev)  # g (and the zeroed outputs) are complete before the library's own streams read and write them
        capi.check(capi.lib().lexls_lsi_batch_solve_adjoint_device(self._h, d_g, d_lb, d_ub))
        return grad_lb, grad_ub

    def solve_adjoint_multi(self, G):
        """lexls_lsi_batch_solve_adjoint_multi: `G` (batch, K, nvar), K cotangents dloss/dx per instance.  Returns (grad_lb, grad_ub), numpy arrays of
        shape (batch, K, total): row c what solve_adjoint(G[:, c]) returns (tolerance contract, the exact zeros at the same entries).  One
        cotangent goes to solve_adjoint."""
        G = np.ascontiguousarray(G, np.float64)
        if G.ndim != 3 or G.shape[0] != self.batch or G.shape[1] == 0 or G.shape[2] != self.nvar:
            raise ValueError(f"solve_adjoint_multi: G has shape {G.shape}, ({self.batch}, K >= 1, {self.nvar}) expected")
        K = G.shape[1]
        if K == 1 and not self._one_cotangent_on_the_multi_entry():
            grad_lb, grad_ub = self.solve_adjoint(G[:, 0, :])
            return grad_lb[:, None, :], grad_ub[:, None, :]
        grad_lb, grad_ub = np.zeros((self.batch, K, self.total)), np.zeros((self.batch, K, self.total))
        capi.check(capi.lib().lexls_lsi_batch_solve_adjoint_multi(self._h, _p(G, C.c_double), K, _p(grad_lb, C.c_double), _p(grad_ub, C.c_double)))
        return grad_lb, grad_ub

    def solve_adjoint_multi_device(self, G, grad_lb=None, grad_ub=None):
        """lexls_lsi_batch_solve_adjoint_multi_device: solve_adjoint_multi() on torch tensors of the batch's device — `G` float64 (batch, K, nvar),
        `grad_lb` and `grad_ub` float64 (batch, K, total), contiguous; an output that is not given is allocated (zeroed).  Returns
        (grad_lb, grad_ub).  Under an instance mask all K rows of a skipped instance keep their bits.  One cotangent goes to
        solve_adjoint_device.  The call waits for the device."""
        import torch
        if not hasattr(G, "data_ptr") or G.dim() != 3 or G.shape[1] == 0:
            raise ValueError("solve_adjoint_multi_device: G must be a tensor of shape (batch, K >= 1, nvar)")
        K = int(G.shape[1])
        d_G = self._device_array("G", G, torch.float64, (self.batch, K, self.nvar), optional=False)
        dev = torch.device("cuda", self.device)
        if grad_lb is None:
            grad_lb = torch.zeros((self.batch, K, self.total), dtype=torch.float64, device=dev)
        if grad_ub is None:
            grad_ub = torch.zeros((self.batch, K, self.total), dtype=torch.float64, device=dev)
        d_lb = self._device_array("grad_lb", grad_lb, torch.float64, (self.batch, K, self.total), optional=False)
        d_ub = self._device_array("grad_ub", grad_ub, torch.float64, (self.batch, K, self.total), optional=False)
        torch.cuda.synchronize(dev)  # G (and the zeroed outputs) are complete before the library's own streams read and write them
        if K == 1 and not self._one_cotangent_on_the_multi_entry():
            capi.check(capi.lib().lexls_lsi_batch_solve_adjoint_device(self._h, d_G, d_lb, d_ub))
        else:
            capi.check(capi.lib().lexls_lsi_batch_solve_adjoint_multi_device(self._h, d_G, K, d_lb, d_ub))
        return grad_lb, grad_ub

    @property
    def per_data(self) -> int:
        """the length of one instance's constraint data in the flat layout of PackedBatch.data (what run_device reads and solve_adjoint_matrix writes)"""
        return int(sum(int(d) * (2 if t == 1 else self.nvar + 2) for d, t in zip(self.dims, self.types)))

    def solve_adjoint_matrix(self, g):
        """lexls_lsi_batch_solve_adjoint_matrix: `g` = dloss/dx of the last run, (batch, nvar).  Returns (grad_data, differentiable): grad_data
        (batch, per_data) float64 in the layout of PackedBatch.data — dloss/d(A, lb, ub) of every objective (split_grad_data gives the
        per-objective views) — and differentiable (batch,) uint8: 1 where the instance ended PROBLEM_SOLVED on a rank-stable final equality
        problem, else 0 with the whole row of grad_data exactly 0 (the bound columns included).  Rows outside the final working set are exactly
        0.  Raises after the runs lambdas() raises after."""
        g = np.ascontiguousarray(g, np.float64)
        if g.shape != (self.batch, self.nvar):
            raise ValueError(f"solve_adjoint_matrix: g has shape {g.shape}, {(self.batch, self.nvar)} expected")
        grad_data, differentiable = np.zeros((self.batch, self.per_data)), np.zeros(self.batch, np.uint8)
        capi.check(capi.lib().lexls_lsi_batch_solve_adjoint_matrix(self._h, _p(g, C.c_double), _p(grad_data, C.c_double), _p(differentiable, C.c_uint8)))
        return grad_data, differentiable

    def solve_adjoint_matrix_device(self, g, grad_data=None, differentiable=None):
        """lexls_lsi_batch_solve_adjoint_matrix_device: solve_adjoint_matrix() on torch tensors of the batch's device — `g` float64 (batch, nvar),
        `grad_data` float64 (batch, per_data), `differentiable` uint8 (batch,), contiguous; an output that is not given is allocated (zeroed).
        Returns (grad_data, differentiable).  Nothing of them passes through host memory.  Under an instance mask the row and the flag of a
        skipped instance keep their bits: pass the tensors that hold them.  The call waits for the device, like run_device()."""
        import torch
        d_g = self._device_array("g", g, torch.float64, (self.batch, self.nvar), optional=False)
        dev = torch.device("cuda", self.device)
        if grad_data is None:
            grad_data = torch.zeros((self.batch, self.per_data), dtype=torch.float64, device=dev)
        if differentiable is None:
            differentiable = torch.zeros((self.batch,), dtype=torch.uint8, device=dev)
        d_out = self._device_array("grad_data", grad_data, torch.float64, (self.batch, self.per_data), optional=False)
        d_flag = self._device_array("differentiable", differentiable, torch.uint8, (self.batch,), optional=False)
        torch.cuda.synchronize(dev)  # g (and the zeroed outputs) are complete before the library's own streams read and write them
        capi.check(capi.lib().lexls_lsi_batch_solve_adjoint_matrix_device(self._h, d_g, d_out, d_flag))
        return grad_data, differentiable

    def solve_tangent(self, ddata):
        """lexls_lsi_batch_solve_tangent: `ddata` (K, batch, per_data), K directions of the constraint data per instance in the layout of
        PackedBatch.data, or (batch, per_data) for one.  Returns (dx, differentiable): dx (K, batch, nvar) — (batch, nvar) for a single direction
        given without the leading axis —, how x of the last run moves along each direction while the working set holds, and differentiable
        (batch,) uint8, the flags of solve_adjoint_matrix: 0 where the instance did not end PROBLEM_SOLVED or its final problem is not
        rank-stable, with exact zeros in its rows of dx.  Rows outside the final working set are never read.  Raises after the runs
        solve_adjoint_matrix() raises after."""
        ddata = np.ascontiguousarray(ddata, np.float64)
        single = ddata.ndim == 2
        if single:
            ddata = ddata[None]
        if ddata.ndim != 3 or ddata.shape[0] == 0 or ddata.shape[1:] != (self.batch, self.per_data):
            raise ValueError(f"solve_tangent: ddata has shape {ddata.shape}, (K >= 1, {self.batch}, {self.per_data}) expected")
        K = ddata.shape[0]
        dx, differentiable = np.zeros((K, self.batch, self.nvar)), np.zeros(self.batch, np.uint8)
        capi.check(capi.lib().lexls_lsi_batch_solve_tangent(self._h, _p(ddata, C.c_double), K, _p(dx, C.c_double), _p(differentiable, C.c_uint8)))
        return (dx[0] if single else dx), differentiable

    def solve_tangent_device(self, ddata, dx=None, differentiable=None):
        """lexls_lsi_batch_solve_tangent_device: solve_tangent() on torch tensors of the batch's device — `ddata` float64 (K, batch, per_data) or
        (batch, per_data), `dx` float64 with the same leading axis and (batch, nvar), `differentiable` uint8 (batch,), contiguous; an output that
        is not given is allocated (zeroed).  Returns (dx, differentiable).  Nothing of them passes through host memory.  Under an instance mask
        the rows and the flag of a skipped instance keep their bits: pass the tensors that hold them.  The call waits for the device."""
        import torch
        if not hasattr(ddata, "dim") or ddata.dim() not in (2, 3):
            raise ValueError("solve_tangent_device: ddata must be a tensor of shape (K >= 1, batch, per_data) or (batch, per_data)")
        lead = () if ddata.dim() == 2 else (int(ddata.shape[0]),)
        K = lead[0] if lead else 1
        if K == 0:
            raise ValueError("solve_tangent_device: K == 0")
        d_in = self._device_array("ddata", ddata, torch.float64, lead + (self.batch, self.per_data), optional=False)
        dev = torch.device("cuda", self.device)
        if dx is None:
            dx = torch.zeros(lead + (self.batch, self.nvar), dtype=torch.float64, device=dev)
        if differentiable is None:
            differentiable = torch.zeros((self.batch,), dtype=torch.uint8, device=dev)
        d_out = self._device_array("dx", dx, torch.float64, lead + (self.batch, self.nvar), optional=False)
        d_flag = self._device_array("differentiable", differentiable, torch.uint8, (self.batch,), optional=False)
        torch.cuda.synchronize(dev)  # ddata (and the zeroed outputs) are complete before the library's own streams read and write them
        capi.check(capi.lib().lexls_lsi_batch_solve_tangent_device(self._h, d_in, K, d_out, d_flag))
        return dx, differentiable

    def solve_bounds(self, lb, ub, with_cost=False):
        """lexls_lsi_batch_solve_bounds: `lb`, `ub` (K, batch, total), K other bound sets per instance in the constraint order of `active` / `v`, or
        (batch, total) for one.  Returns (x, violation, valid): x (K, batch, nvar) — (batch, nvar) for a single set given without the leading
        axis —, the solution of every instance's final working set of the last run with its bounds replaced; violation (K, batch) / (batch,), the
        largest amount by which that x breaks a bound of the set, over all rows of all objectives; valid (batch,) uint8, 1 where the instance
        ended PROBLEM_SOLVED, else 0 with exact zeros in its rows of x and violation.  A small violation is necessary for the working set to
        remain the answer under the new bounds, not sufficient: the multipliers' signs are not re-examined.  Nothing is factorized again.
        Raises after the runs solve_tangent() raises after.
        with_cost=True (lexls_lsi_batch_solve_bounds_cost): returns (x, violation, valid, cost), cost (K, batch, nObj) / (batch, nObj) = per
        objective the sum over its rows of max(lb - a.x, a.x - ub, 0)^2 at that x against that bound set: what lex_argmin() ranks."""
        lb, ub = np.ascontiguousarray(lb, np.float64), np.ascontiguousarray(ub, np.float64)
        single = lb.ndim == 2
        if single:
            lb, ub = lb[None], (ub[None] if ub.ndim == 2 else ub)
        if lb.ndim != 3 or lb.shape[0] == 0 or lb.shape[1:] != (self.batch, self.total) or ub.shape != lb.shape:
            raise ValueError(f"solve_bounds: lb / ub have shapes {lb.shape} / {ub.shape}, (K >= 1, {self.batch}, {self.total}) expected for both")
        K = lb.shape[0]
        x, violation, valid = np.zeros((K, self.batch, self.nvar)), np.zeros((K, self.batch)), np.zeros(self.batch, np.uint8)
        if with_cost:
            cost = np.zeros((K, self.batch, len(self.dims)))
            capi.check(capi.lib().lexls_lsi_batch_solve_bounds_cost(self._h, _p(lb, C.c_double), _p(ub, C.c_double), K, _p(x, C.c_double), _p(violation, C.c_double),
                                                                    _p(cost, C.c_double), _p(valid, C.c_uint8)))
            return (x[0], violation[0], valid, cost[0]) if single else (x, violation, valid, cost)
        capi.check(capi.lib().lexls_lsi_batch_solve_bounds(self._h, _p(lb, C.c_double), _p(ub, C.c_double), K, _p(x, C.c_double), _p(violation, C.c_double),
                                                           _p(valid, C.c_uint8)))
        return (x[0], violation[0], valid) if single else (x, violation, valid)

    def solve_bounds_device(self, lb, ub, x=None, violation=None, valid=None, cost=None):
        """lexls_lsi_batch_solve_bounds_device: solve_bounds() on torch tensors of the batch's device — `lb`, `ub` float64 (K, batch, total) or
        (batch, total), `x` float64 with the same leading axis and (batch, nvar), `violation` float64 of the leading axis and (batch,), `valid`
        uint8 (batch,), contiguous; an output that is not given is allocated (zeroed).  Returns (x, violation, valid).  Nothing of them passes
        through host memory.  Under an instance mask the rows and the flag of a skipped instance keep their bits: pass the tensors that hold
        them.  The call waits for the device.
        cost= a float64 tensor of the leading axis and (batch, nObj), or True to have one allocated (lexls_lsi_batch_solve_bounds_cost_device):
        returns (x, violation, valid, cost), cost as solve_bounds(with_cost=True) describes it."""
        import torch
        if not hasattr(lb, "dim") or lb.dim() not in (2, 3) or not hasattr(ub, "dim") or ub.dim() != lb.dim():
            raise ValueError("solve_bounds_device: lb and ub must be tensors of shape (K >= 1, batch, total) or (batch, total)")
        lead = () if lb.dim() == 2 else (int(lb.shape[0]),)
        K = lead[0] if lead else 1
        if K == 0:
            raise ValueError("solve_bounds_device: K == 0")
        d_lb = self._device_array("lb", lb, torch.float64, lead + (self.batch, self.total), optional=False)
        d_ub = self._device_array("ub", ub, torch.float64, lead + (self.batch, self.total), optional=False)
        dev = torch.device("cuda", self.device)
        if x is None:
            x = torch.zeros(lead + (self.batch, self.nvar), dtype=torch.float64, device=dev)
        if violation is None:
            violation = torch.zeros(lead + (self.batch,), dtype=torch.float64, device=dev)
        if valid is None:
            valid = torch.zeros((self.batch,), dtype=torch.uint8, device=dev)
        d_x = self._device_array("x", x, torch.float64, lead + (self.batch, self.nvar), optional=False)
        d_viol = self._device_array("violation", violation, torch.float64, lead + (self.batch,), optional=False)
        d_valid = self._device_array("valid", valid, torch.uint8, (self.batch,), optional=False)
        if cost is not None and cost is not False:
            if cost is True:
                cost = torch.zeros(lead + (self.batch, len(self.dims)), dtype=torch.float64, device=dev)
            d_cost = self._device_array("cost", cost, torch.float64, lead + (self.batch, len(self.dims)), optional=False)
            torch.cuda.synchronize(dev)
            capi.check(capi.lib().lexls_lsi_batch_solve_bounds_cost_device(self._h, d_lb, d_ub, K, d_x, d_viol, d_cost, d_valid))
            return x, violation, valid, cost
        torch.cuda.synchronize(dev)  # the bounds (and the zeroed outputs) are complete before the library's own streams read and write them
        capi.check(capi.lib().lexls_lsi_batch_solve_bounds_device(self._h, d_lb, d_ub, K, d_x, d_viol, d_valid))
        return x, violation, valid

    def last_consumer_kernel(self) -> str:
        """the kernel variant of the last solve_bounds() / solve_bounds_device() call (lexls_lsi_batch_last_consumer_kernel):
        "lsi_bounds_check<lds>" or "lsi_bounds_check<hbm>" ("lsi_bounds_cost<lds>" / "<hbm>" when the cost was asked for); "" before the first such call"""
        return capi.lib().lexls_lsi_batch_last_consumer_kernel(self._h).decode()

    def split_grad_data(self, row):
        """one instance's row of grad_data (or of the data itself) as the list of per-objective dict(A=, lb=, ub=) (simple bounds: lb, ub): the
        inverse of flatten(), by unflatten()"""
        row = row.detach().cpu().numpy() if hasattr(row, "detach") else np.asarray(row, float)
        objs = unflatten(self.nvar, self.dims, self.types, row, var_index=np.zeros(int(self.dims[0]), np.uint32))
        return [{k: v for k, v in o.items() if k != "var"} for o in objs]

    def jacobian_bounds_device(self):
        """(dx_dlb, dx_dub), torch tensors of shape (batch, nvar, total) on the batch's device: d x_i / d lb_r and d x_i / d ub_r of the last run
        with the matrices held fixed, from the identity cotangents through solve_adjoint_multi_device — the Jacobian of the piece of the
        piecewise-affine map the solve ended on; zero for instances that did not end PROBLEM_SOLVED."""
        import torch
        dev = torch.device("cuda", self.device)
        G = torch.eye(self.nvar, dtype=torch.float64, device=dev).expand(self.batch, self.nvar, self.nvar).contiguous()
        return self.solve_adjoint_multi_device(G)

    def lambdas(self):
        """per instance the list of per-objective (dim_k x nObj) multiplier matrices that frontend.lexlsi(..., debug=True) returns as
        d["lambda"] (LexLSI::getLambda, lexlsi.h:552-605), for the last run"""
        lam = self.lambda_array()
        cuts = np.cumsum(self.dims)[:-1]
        return [np.split(np.ascontiguousarray(m.T), cuts) for m in lam]


def lex_argmin(cost, tol=0.0):
    """Per instance the index of the lexicographically smallest of K candidates: `cost` (K, batch, nObj) as LsiBatch.solve_bounds(with_cost=True)
    or BatchedLexLSE.residual_rhs() return it (numpy array or torch tensor), level 0 the most important.  Level by level, the candidates still in
    the running are those within `tol` (absolute, the caller's choice) of the smallest cost among them at that level; the first of those left
    after the last level wins.  Returns (batch,) int64 indices (numpy for numpy, torch for torch).  Plain array operations, no kernel."""
    if hasattr(cost, "detach"):
        import torch
        if cost.dim() != 3 or cost.shape[0] == 0:
            raise ValueError(f"lex_argmin: cost must have shape (K >= 1, batch, nObj), got {tuple(cost.shape)}")
        alive = torch.ones(cost.shape[:2], dtype=torch.bool, device=cost.device)
        inf = torch.full((), float("inf"), dtype=cost.dtype, device=cost.device)
        for k in range(cost.shape[2]):
            level = torch.where(alive, cost[:, :, k], inf)
            alive = alive & (level <= level.min(dim=0).values + tol)
        return alive.to(torch.uint8).argmax(dim=0)
    cost = np.asarray(cost, float)
    if cost.ndim != 3 or cost.shape[0] == 0:
        raise ValueError(f"lex_argmin: cost must have shape (K >= 1, batch, nObj), got {cost.shape}")
    alive = np.ones(cost.shape[:2], bool)
    for k in range(cost.shape[2]):
        level = np.where(alive, cost[:, :, k], np.inf)
        alive &= level <= level.min(axis=0) + tol
    return alive.argmax(axis=0).astype(np.int64)


def lsi_batch_solve(nvar: int, problems, active_guess=None, x0=None, device: int = 0, regularization_factors=None, with_lambda: bool = False, **params):
    """Lock-step batch of LexLSI problems of one structure (BASELINE configs[4]).  `problems`: list of objective lists
    (same dims / types) or a PackedBatch; `active_guess`: per problem list of per-objective flag arrays, a (batch, total) uint8
    array, or None; `x0`: (batch, nvar) or None.  One-shot form of LsiBatch (create + run + destroy).  with_lambda: the result also
    has "lambda", per instance the matrices of LsiBatch.lambdas()."""
    pk = problems if isinstance(problems, PackedBatch) else pack_batch(nvar, problems)
    b = LsiBatch(nvar, pk.dims, pk.types, pk.batch, device=device)
    try:
        r = b.run(pk, active_guess=active_guess, x0=x0, regularization_factors=regularization_factors, **params)
        if with_lambda:
            r["lambda"] = b.lambdas()
        return r
    finally:
        b.close()
