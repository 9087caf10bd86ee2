"""The LexLSE solve as a differentiable torch operation in its right-hand sides, the matrix held fixed.

factorize() chooses its pivots and tests the ranks on the columns of A alone, so for fixed A the basic solution is exactly affine in the
right-hand sides: x = M b (+ N x_fixed).  ``SolveRhs`` solves on the device from torch tensors and, in the backward pass, returns
M^T (dloss/dx) from one pass over the kept factor (lexls_lse_solve_adjoint_device).  There are no derivatives with respect to A — x is not
continuous in A where a rank changes — and asking for them raises instead of returning zeros.  A damped solve (regularization type 1, 3, 4, 5, 8
or 9 with constant factors) is still affine in b with A and the factors held fixed, and ``SolveRhs`` differentiates it the same way once
the handle's ``set_adjoint_regularized()`` switched that on; the
factors are constants of the graph.

``SolveLod`` is the operation that does differentiate with respect to A: it takes the whole problem data (matrices and right-hand sides) as one
tensor and returns, in the backward pass, the gradient of both (lexls_lse_solve_adjoint_matrix_device) for the rank-stable problems of the
batch, with a per-problem flag and zeros for the others.

``SolveBounds`` is the same for a batch of LexLSI problems in their bounds: at a solved instance x is the basic solution of the equality
problem of the final working set, affine in the active bounds while that set holds.  Forward is LsiBatch.run_device, backward
LsiBatch.solve_adjoint_device (lexls_lsi_batch_solve_adjoint_device).

``SolveData`` differentiates a LexLSI batch with respect to ALL its constraint data — the matrices A and the bounds, one tensor in the layout of
LsiBatch.run_device — where the final equality problem of an instance is rank-stable (lexls_lsi_batch_solve_adjoint_matrix_device), with a
per-instance flag and zeros for the others.

``jacobian_rhs`` and ``jacobian_bounds`` return the whole Jacobians, dx/db and dx/dlb, dx/dub, from one multi-cotangent pass
(lexls_lse_solve_adjoint_multi_device: lane = cotangent) instead of nVar backward passes.

``jvp_lod`` is the forward mode of ``SolveLod``: the tangents of x along K directions of the problem data in one pass
(lexls_lse_solve_tangent_device), where ``SolveLod`` would need nVar backward passes for the same quantity; ``jvp_data`` is the same for
``SolveData`` (lexls_lsi_batch_solve_tangent_device).

``solve_new_bounds`` is the finite-step counterpart of ``SolveBounds`` on a batch that has run: x of the final working sets under K other bound
sets per instance (lexls_lsi_batch_solve_bounds_device, nothing is factorized again) with the violation of each answer, differentiable in the
bounds through one lexls_lsi_batch_solve_adjoint_multi_device call.

torch is imported when the operation is first used, not with the package.
"""
from __future__ import annotations


class _Span:  # the CUDA array interface over memory this object does not own
    def __init__(self, address, shape):
        self.__cuda_array_interface__ = dict(shape=shape, typestr="<f8", data=(int(address), False), version=2, strides=None)


_SOLVE_RHS = None


def _solve_rhs_class():
    global _SOLVE_RHS
    if _SOLVE_RHS is not None:
        return _SOLVE_RHS
    import torch

    class SolveRhs(torch.autograd.Function):
        """x = SolveRhs.apply(rhs, lse, lod): rhs (batch, cap) float64 on the device, lse a BatchedLexLSE of that shape (dimensions, fixed
        variables, tolerance and regularization set by the caller: none, or, after lse.set_adjoint_regularized(), type 1, 3, 4, 5, 8 or 9 with
        constant factors — the factors are
        constants of the graph, held fixed as A is, and get no gradient; the CG types 2 and 6, type 7 and a variable factor make backward
        raise), lod (batch, nVar + 1, cap) float64 on the same device.  rhs is copied
        into the last column of lod (lod is the handle's input from then on: it must stay alive and unchanged until backward has run), the
        batch is factorized and solved with the factor kept, and x (batch, nVar) comes back as a new tensor.  Gradient: rhs only."""

        @staticmethod
        def forward(ctx, rhs, lse, lod):
            if lod.requires_grad:
                raise ValueError("SolveRhs: lod requires grad, but the solve has no derivatives with respect to A (x is not continuous in A "
                                 "at rank changes); detach lod")
            shape = (lse.batch, lse.nVar + 1, lse.cap)
            if tuple(lod.shape) != shape or lod.dtype != torch.float64 or not lod.is_cuda or not lod.is_contiguous():
                raise ValueError(f"SolveRhs: lod must be a contiguous float64 device tensor of shape {shape}")
            if tuple(rhs.shape) != (lse.batch, lse.cap) or rhs.dtype != torch.float64 or rhs.device != lod.device:
                raise ValueError(f"SolveRhs: rhs must be a float64 tensor of shape {(lse.batch, lse.cap)} on lod's device")
            lse.set_stream(torch.cuda.current_stream(lod.device).cuda_stream)
            lod[:, lse.nVar, :] = rhs.detach()
            lse.setProblemDevice(lod.data_ptr())
            lse.factorize_solve(keep_factor=True)
            x = torch.as_tensor(_Span(lse.device_ptr("x"), (lse.batch, lse.nVar)), device=lod.device).clone()
            ctx.lse, ctx.lod = lse, lod
            return x

        @staticmethod
        def backward(ctx, grad_x):
            lse = ctx.lse
            g = grad_x.contiguous()
            grad_rhs = torch.empty((lse.batch, lse.cap), dtype=torch.float64, device=g.device)
            lse.set_stream(torch.cuda.current_stream(g.device).cuda_stream)
            lse.solve_adjoint_device(g, grad_rhs)
            return grad_rhs, None, None

    _SOLVE_RHS = SolveRhs
    return SolveRhs


_SOLVE_BOUNDS = None


def _solve_bounds_class():
    global _SOLVE_BOUNDS
    if _SOLVE_BOUNDS is not None:
        return _SOLVE_BOUNDS
    import torch
    from torch.autograd.function import once_differentiable

    def write_bounds_and_run(lb, ub, batch, data, var_index, active_guess, x0, params):
        """lb / ub into the bound columns of data (per objective a column-major dim x w block, the last two columns), then run_device"""
        off = first = 0
        for d, t in zip((int(d) for d in batch.dims), (int(t) for t in batch.types)):
            w = 2 if t == 1 else batch.nvar + 2
            data[:, off + (w - 2) * d:off + (w - 1) * d] = lb[:, first:first + d]
            data[:, off + (w - 1) * d:off + w * d] = ub[:, first:first + d]
            off, first = off + d * w, first + d
        return batch.run_device(data, var_index=var_index, active_guess=active_guess, x0=x0, **params)

    class SolveBounds(torch.autograd.Function):
        """x = SolveBounds.apply(lb, ub, batch, data, var_index, active_guess, x0, params, out): lb and ub (batch, sum(dims)) float64 on the device,
        batch an LsiBatch, data (batch, per-instance data) float64 on the same device in the layout of LsiBatch.run_device — lb and ub are written
        into its bound columns, in place.  var_index / active_guess / x0 as for run_device (or None), params a dict of its keyword parameters (or
        None), out a dict that receives run_device's result (or None).  Forward: run_device; x (batch, nVar) comes back.  Backward:
        solve_adjoint_device — the gradient of the piece of the piecewise-affine map the solve ended on, zero for instances that did not end
        PROBLEM_SOLVED.  Gradients: lb and ub only.  The backward pass reads the state the forward run left in `batch`; when the batch has run
        again in between, the forward run is repeated from the saved bounds first (data is written again).  Regularized runs: after
        batch.set_adjoint_regularized(), types 1, 3, 4, 5, 8 and 9 with constant factors are differentiated too (the damped final problem);
        the factors, shared or per instance, are constants of the graph.  Without it, and for the other types, backward raises."""

        @staticmethod
        def forward(ctx, lb, ub, batch, data, var_index=None, active_guess=None, x0=None, params=None, out=None):
            if data.requires_grad:
                raise ValueError("SolveBounds: data requires grad, but the solve has no derivatives with respect to A here (the matrices are held "
                                 "fixed); detach data, or use solve_data for the gradient with respect to the whole constraint data")
            shape = (batch.batch, batch.total)
            for name, t in (("lb", lb), ("ub", ub)):
                if tuple(t.shape) != shape or t.dtype != torch.float64 or t.device != data.device:
                    raise ValueError(f"SolveBounds: {name} must be a float64 tensor of shape {shape} on data's device")
            params = dict(params or {})
            lb0, ub0 = lb.detach().clone(), ub.detach().clone()
            r = write_bounds_and_run(lb0, ub0, batch, data, var_index, active_guess, x0, params)
            if out is not None:
                out.update(r)
            ctx.batch, ctx.serial = batch, batch._run_serial
            ctx.rerun = (lb0, ub0, data, var_index, active_guess, x0, params)
            return r["x"]

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_x):
            batch = ctx.batch
            if batch._run_serial != ctx.serial:  # another run has replaced the state this pass reads: the same run again
                lb0, ub0, data, var_index, active_guess, x0, params = ctx.rerun
                write_bounds_and_run(lb0, ub0, batch, data, var_index, active_guess, x0, params)
                ctx.serial = batch._run_serial
            grad_lb, grad_ub = batch.solve_adjoint_device(grad_x.contiguous())
            return grad_lb, grad_ub, None, None, None, None, None, None, None

    _SOLVE_BOUNDS = SolveBounds
    return SolveBounds


_SOLVE_DATA = None


def _solve_data_class():
    global _SOLVE_DATA
    if _SOLVE_DATA is not None:
        return _SOLVE_DATA
    import torch
    from torch.autograd.function import once_differentiable

    class SolveData(torch.autograd.Function):
        """x = SolveData.apply(data, batch, var_index, active_guess, x0, params, out): data (batch, per-instance data) float64 on the device in the
        layout of LsiBatch.run_device — the matrices and the bounds of every objective; batch an LsiBatch; var_index / active_guess / x0 as for
        run_device (or None), params a dict of its keyword parameters (or None), out a dict that receives run_device's result (or None).
        Forward: run_device on a copy of data (kept for the backward pass); x (batch, nVar) comes back.  Backward: solve_adjoint_matrix_device —
        grad_data, one tensor for A, lb and ub: the gradient of the piece of the map the solve ended on.  An instance that did not end
        PROBLEM_SOLVED, or whose final equality problem is not rank-stable, has a zero row, and `batch.differentiable` — a (batch,) uint8 device
        tensor set by backward — is 0 there.  The backward pass reads the state the forward run left in `batch`; when the batch has run again
        in between, the forward run is repeated from the saved data first."""

        @staticmethod
        def forward(ctx, data, batch, var_index=None, active_guess=None, x0=None, params=None, out=None):
            shape = (batch.batch, batch.per_data)
            if tuple(data.shape) != shape or data.dtype != torch.float64 or not data.is_cuda:
                raise ValueError(f"SolveData: data must be a float64 device tensor of shape {shape}")
            params = dict(params or {})
            data0 = data.detach().clone().contiguous()
            r = batch.run_device(data0, var_index=var_index, active_guess=active_guess, x0=x0, **params)
            if out is not None:
                out.update(r)
            ctx.batch, ctx.serial = batch, batch._run_serial
            ctx.rerun = (data0, var_index, active_guess, x0, params)
            return r["x"]

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_x):
            batch = ctx.batch
            if batch._run_serial != ctx.serial:  # another run has replaced the state this pass reads: the same run again
                data0, var_index, active_guess, x0, params = ctx.rerun
                batch.run_device(data0, var_index=var_index, active_guess=active_guess, x0=x0, **params)
                ctx.serial = batch._run_serial
            grad_data, batch.differentiable = batch.solve_adjoint_matrix_device(grad_x.contiguous())
            return grad_data, None, None, None, None, None, None

    _SOLVE_DATA = SolveData
    return SolveData


_SOLVE_LOD = None


def _solve_lod_class():
    global _SOLVE_LOD
    if _SOLVE_LOD is not None:
        return _SOLVE_LOD
    import torch
    from torch.autograd.function import once_differentiable

    class SolveLod(torch.autograd.Function):
        """x = SolveLod.apply(lod, lse): lod (batch, nVar + 1, cap) float64 on the device, the matrices and the right-hand sides in the layout of
        setProblem; lse a BatchedLexLSE of that shape (dimensions, fixed variables and tolerance set by the caller; no regularization).  Forward
        binds lod as the handle's input without a copy (setProblemDevice: it must stay alive and unchanged until backward has run), factorizes
        with the factor kept and solves; x (batch, nVar) comes back as a new tensor.  Backward returns grad_lod (batch, nVar + 1, cap) from
        lexls_lse_solve_adjoint_matrix_device: one tensor carries the gradients of both A and b.  A problem that is not rank-stable has no
        derivative with respect to A: its slice of grad_lod is zero, and `lse.differentiable` — a (batch,) uint8 device tensor set by backward —
        is 0 there."""

        @staticmethod
        def forward(ctx, lod, lse):
            shape = (lse.batch, lse.nVar + 1, lse.cap)
            if tuple(lod.shape) != shape or lod.dtype != torch.float64 or not lod.is_cuda or not lod.is_contiguous():
                raise ValueError(f"SolveLod: lod must be a contiguous float64 device tensor of shape {shape}")
            lse.set_stream(torch.cuda.current_stream(lod.device).cuda_stream)
            lse.setProblemDevice(lod.data_ptr())
            lse.factorize_solve(keep_factor=True)
            x = torch.as_tensor(_Span(lse.device_ptr("x"), (lse.batch, lse.nVar)), device=lod.device).clone()
            ctx.lse, ctx.lod = lse, lod
            return x

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_x):
            lse = ctx.lse
            g = grad_x.contiguous()
            grad_lod = torch.empty((lse.batch, lse.nVar + 1, lse.cap), dtype=torch.float64, device=g.device)
            lse.differentiable = torch.empty((lse.batch,), dtype=torch.uint8, device=g.device)
            lse.set_stream(torch.cuda.current_stream(g.device).cuda_stream)
            lse.solve_adjoint_matrix_device(g, grad_lod, lse.differentiable)
            return grad_lod, None

    _SOLVE_LOD = SolveLod
    return SolveLod


def __getattr__(name):
    if name == "SolveRhs":
        return _solve_rhs_class()
    if name == "SolveNewRhs":
        return _solve_new_rhs_class()
    if name == "SolveLod":
        return _solve_lod_class()
    if name == "SolveBounds":
        return _solve_bounds_class()
    if name == "SolveData":
        return _solve_data_class()
    if name == "SolveNewBounds":
        return _solve_new_bounds_class()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def solve_rhs(rhs, lse, lod):
    """SolveRhs.apply(rhs, lse, lod)"""
    return _solve_rhs_class().apply(rhs, lse, lod)


_SOLVE_NEW_RHS = None


def _solve_new_rhs_class():
    global _SOLVE_NEW_RHS
    if _SOLVE_NEW_RHS is not None:
        return _SOLVE_NEW_RHS
    import torch

    class SolveNewRhs(torch.autograd.Function):
        """x = SolveNewRhs.apply(rhs, fixed, solver): rhs (K, batch, cap) float64 on the device, fixed (K, batch, nVar) or None (the values the
        handle holds), solver a BatchedLexLSE that keeps a factor (plain, or damped with type 1, 3, 4, 5, 8 or 9 and constant factors).  Forward
        is lexls_lse_solve_rhs_device — no factorization —, backward lexls_lse_solve_adjoint_multi_device on the same factor (after a damped
        factorization the handle needs set_adjoint_regularized_multi()).  Gradients: rhs and fixed; first order only."""

        @staticmethod
        def forward(ctx, rhs, fixed, solver):
            rhs = rhs.detach().contiguous()
            x = torch.empty(tuple(rhs.shape[:-1]) + (solver.nVar,), dtype=torch.float64, device=rhs.device)
            solver.set_stream(torch.cuda.current_stream(rhs.device).cuda_stream)
            solver.solve_rhs_device(rhs, x, None if fixed is None else fixed.detach().contiguous())
            ctx.solver, ctx.with_fixed = solver, fixed is not None
            return x

        @staticmethod
        def backward(ctx, grad_x):
            solver = ctx.solver
            G = grad_x.reshape((-1, solver.batch, solver.nVar)).transpose(0, 1).contiguous()  # (batch, K, nVar): the adjoint's layout
            K = G.shape[1]
            grad_rhs = torch.empty((solver.batch, K, solver.cap), dtype=torch.float64, device=G.device)
            grad_fixed = torch.empty((solver.batch, K, solver.nVar), dtype=torch.float64, device=G.device) if ctx.with_fixed else None
            solver.set_stream(torch.cuda.current_stream(G.device).cuda_stream)
            solver.solve_adjoint_multi_device(G, grad_rhs, grad_fixed)
            lead = tuple(grad_x.shape[:-1])
            return (grad_rhs.transpose(0, 1).reshape(lead + (solver.cap,)),
                    grad_fixed.transpose(0, 1).reshape(lead + (solver.nVar,)) if ctx.with_fixed else None, None)

    _SOLVE_NEW_RHS = SolveNewRhs
    return SolveNewRhs


def solve_new_rhs(solver, rhs, fixed=None):
    """The solutions of K new right-hand sides `rhs` (K, batch, cap) — or (batch, cap) for one — and fixed values `fixed` (the same leading
    axis, batch, nVar; None: the handle's) on the factor the BatchedLexLSE `solver` keeps, differentiable in both (SolveNewRhs).  Named
    solve_new_rhs because solve_rhs(rhs, lse, lod), the factorizing operation, keeps its name and signature."""
    return _solve_new_rhs_class().apply(rhs, fixed, solver)


def jvp_rhs(solver, drhs, dfixed=None):
    """Forward-mode derivative of the kept factor's solve with respect to b and the fixed values, valid on damped factors too: x = M b + N x_fixed
    is linear, so its derivative along (drhs, dfixed) is THE SAME CALL with the constant part removed — lexls_lse_solve_rhs_device on drhs with
    zeros passed for the fixed values where dfixed is None (None would mean the handle's own values, which are the constant part).  drhs
    (K, batch, cap) / (batch, cap), dfixed the same leading axis x (batch, nVar); returns dx of drhs' leading shape x nVar."""
    import torch
    drhs = drhs.contiguous()
    lead = tuple(drhs.shape[:-1])
    dfixed = torch.zeros(lead + (solver.nVar,), dtype=torch.float64, device=drhs.device) if dfixed is None else dfixed.contiguous()
    dx = torch.empty(lead + (solver.nVar,), dtype=torch.float64, device=drhs.device)
    solver.set_stream(torch.cuda.current_stream(drhs.device).cuda_stream)
    solver.solve_rhs_device(drhs, dx, dfixed)
    return dx


def solve_lod(solver, lod):
    """SolveLod.apply(lod, solver): the solutions of the batch `lod` (batch, nVar + 1, cap) on the BatchedLexLSE `solver`, differentiable in the
    matrices and the right-hand sides where the problems are rank-stable"""
    return _solve_lod_class().apply(lod, solver)


def jvp_lod(solver, lod, dlod, dfixed=None):
    """Forward mode of solve_lod: (x, dx) for the batch `lod` (batch, nVar + 1, cap) on the BatchedLexLSE `solver` and the directions `dlod`
    (K, batch, nVar + 1, cap) — or (batch, nVar + 1, cap) for one —, float64 device tensors; `dfixed` (the same leading axis, batch, nVar): the
    tangents of the fixed values, None for zeros.  dx (K, batch, nVar) / (batch, nVar) is the Jacobian-vector product dx/d[A | b] . dlod of the
    rank-stable problems (lexls_lse_solve_tangent_device: one pass over the directions, no host copy); the flags are left in
    `solver.differentiable`, where solve_lod's backward pass leaves them, and a problem with flag 0 has dx = 0.  `lod` is bound without a copy and
    has to stay alive and unchanged while the solver keeps this factor."""
    import torch
    shape = (solver.batch, solver.nVar + 1, solver.cap)
    if tuple(lod.shape) != shape or lod.dtype != torch.float64 or not lod.is_cuda or not lod.is_contiguous():
        raise ValueError(f"jvp_lod: lod must be a contiguous float64 device tensor of shape {shape}")
    dev = lod.device
    solver.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    solver.setProblemDevice(lod.data_ptr())
    solver.factorize_solve(keep_factor=True)
    x = torch.as_tensor(_Span(solver.device_ptr("x"), (solver.batch, solver.nVar)), device=dev).clone()
    dlod = dlod.contiguous()
    dx = torch.empty(tuple(dlod.shape[:-2]) + (solver.nVar,), dtype=torch.float64, device=dev)
    solver.differentiable = torch.empty((solver.batch,), dtype=torch.uint8, device=dev)
    solver.solve_tangent_device(dlod, dx, None if dfixed is None else dfixed.contiguous(), solver.differentiable)
    return x, dx


def jvp_data(batch, data, ddata, var_index=None, active_guess=None, x0=None, out=None, **params):
    """Forward mode of solve_data: (x, dx) for the LexLSI batch `batch` on the constraint data `data` (batch, per_data) and the directions `ddata`
    (K, batch, per_data) — or (batch, per_data) for one —, float64 device tensors.  run_device on a copy of `data` (`params`: its keyword
    parameters; `out`: a dict that receives its result), then lexls_lsi_batch_solve_tangent_device: dx (K, batch, nVar) / (batch, nVar) is the
    Jacobian-vector product of the instances that ended PROBLEM_SOLVED on a rank-stable final problem, while their working sets hold; nothing
    passes through host memory.  The flags are left in `batch.differentiable`, where solve_data's backward pass leaves them; an instance with
    flag 0 has dx = 0."""
    res = batch.run_device(data.detach().clone(), var_index=var_index, active_guess=active_guess, x0=x0, **params)
    if out is not None:
        out.update(res)
    dx, batch.differentiable = batch.solve_tangent_device(ddata.contiguous())
    return res["x"], dx


def solve_bounds(lb, ub, batch, data, var_index=None, active_guess=None, x0=None, out=None, **params):
    """SolveBounds.apply(lb, ub, batch, data, var_index, active_guess, x0, params, out): the solutions of a LexLSI batch, differentiable in the
    bounds.  `params`: the keyword parameters of LsiBatch.run_device; `out`: a dict that receives its result ("x", "info", "active", "v")."""
    return _solve_bounds_class().apply(lb, ub, batch, data, var_index, active_guess, x0, params, out)


_SOLVE_NEW_BOUNDS = None


def _solve_new_bounds_class():
    global _SOLVE_NEW_BOUNDS
    if _SOLVE_NEW_BOUNDS is not None:
        return _SOLVE_NEW_BOUNDS
    import torch

    class SolveNewBounds(torch.autograd.Function):
        """x, violation = SolveNewBounds.apply(lb, ub, batch): lb, ub (K, batch, total) float64 on the device, batch an LsiBatch whose last run
        lexls_lsi_batch_solve_bounds serves.  Forward is lexls_lsi_batch_solve_bounds_device — no factorization, no active-set iteration —; the
        flags are left in `batch.valid`.  The map from the bounds to x is the run's own while the working set holds, so backward is one
        lexls_lsi_batch_solve_adjoint_multi_device call with K cotangents per instance.  Gradients: lb and ub, of x only — violation is not
        differentiable; first order only."""

        @staticmethod
        def forward(ctx, lb, ub, batch):
            x, violation, batch.valid = batch.solve_bounds_device(lb.detach().contiguous(), ub.detach().contiguous())
            ctx.batch = batch
            ctx.mark_non_differentiable(violation)
            return x, violation

        @staticmethod
        def backward(ctx, grad_x, _grad_violation):
            batch = ctx.batch
            G = grad_x.reshape((-1, batch.batch, batch.nvar)).transpose(0, 1).contiguous()  # (batch, K, nvar): the adjoint's layout
            grad_lb, grad_ub = batch.solve_adjoint_multi_device(G)
            shape = tuple(grad_x.shape[:-1]) + (batch.total,)
            return grad_lb.transpose(0, 1).reshape(shape), grad_ub.transpose(0, 1).reshape(shape), None

    _SOLVE_NEW_BOUNDS = SolveNewBounds
    return SolveNewBounds


def solve_new_bounds(batch, lb, ub):
    """(x, violation) of the LsiBatch `batch`'s last run under K other bound sets per instance: `lb`, `ub` (K, batch, total) — or (batch, total) for
    one — float64 device tensors in the constraint order of `active`; x has their leading shape x nvar, violation their leading shape
    (LsiBatch.solve_bounds_device; the flags are left in `batch.valid`).  x is differentiable in lb and ub (SolveNewBounds); violation is not.  A
    small violation is necessary for the working set to remain the answer, not sufficient.  Named solve_new_bounds because
    solve_bounds(lb, ub, batch, data, ...), the operation that runs the active-set method, keeps its name and signature."""
    return _solve_new_bounds_class().apply(lb, ub, batch)


def solve_data(batch, data, var_index=None, active_guess=None, x0=None, out=None, **params):
    """SolveData.apply(data, batch, var_index, active_guess, x0, params, out): the solutions of a LexLSI batch, differentiable in the whole
    constraint data (A, lb and ub of every objective) where the final equality problems are rank-stable; the flags are left in
    `batch.differentiable` by the backward pass.  `params`: the keyword parameters of LsiBatch.run_device; `out`: a dict that receives its result."""
    return _solve_data_class().apply(data, batch, var_index, active_guess, x0, params, out)


def jacobian_rhs(lse):
    """(dx_db (batch, nVar, cap), dx_dfixed (batch, nVar, nVar)) of the factor `lse` keeps (BatchedLexLSE.jacobian_device): what nVar backward
    passes of SolveRhs with the unit cotangents would return, from one multi-cotangent pass.  The matrix is held fixed.  A damped factor (regularization
    type 1, 3, 4, 5, 8 or 9, constant factors) is served once lse.set_adjoint_regularized_multi() is on: the Jacobians of the damped solve."""
    return lse.jacobian_device()


def jacobian_bounds(batch):
    """(dx_dlb, dx_dub), each (batch, nVar, total), of the last run of the LsiBatch `batch` (LsiBatch.jacobian_bounds_device): what nVar backward
    passes of SolveBounds with the unit cotangents would return, from one multi-cotangent pass.  The matrices are held fixed.  A regularized
    run is served when batch.set_adjoint_regularized_multi() was on before it: the Jacobians of the damped final problem."""
    return batch.jacobian_bounds_device()
