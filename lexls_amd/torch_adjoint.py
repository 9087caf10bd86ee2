"""The LexLSE solve as a differentiable torch operation in its right-hand sides, the matrix held fixed.

factorize() chooses its pivots and tests the ranks on the columns of A alone, so for fixed A the basic solution is exactly affine in the
right-hand sides: x = M b (+ N x_fixed).  ``SolveRhs`` solves on the device from torch tensors and, in the backward pass, returns
M^T (dloss/dx) from one pass over the kept factor (lexls_lse_solve_adjoint_device).  There are no derivatives with respect to A — x is not
continuous in A where a rank changes — and asking for them raises instead of returning zeros.

torch is imported when the operation is first used, not with the package.
"""
from __future__ import annotations

_SOLVE_RHS = None


def _solve_rhs_class():
    global _SOLVE_RHS
    if _SOLVE_RHS is not None:
        return _SOLVE_RHS
    import torch

    class _Span:  # the CUDA array interface over memory this object does not own
        def __init__(self, address, shape):
            self.__cuda_array_interface__ = dict(shape=shape, typestr="<f8", data=(int(address), False), version=2, strides=None)

    class SolveRhs(torch.autograd.Function):
        """x = SolveRhs.apply(rhs, lse, lod): rhs (batch, cap) float64 on the device, lse a BatchedLexLSE of that shape (dimensions, fixed
        variables and tolerance set by the caller; no regularization), lod (batch, nVar + 1, cap) float64 on the same device.  rhs is copied
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


def __getattr__(name):
    if name == "SolveRhs":
        return _solve_rhs_class()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def solve_rhs(rhs, lse, lod):
    """SolveRhs.apply(rhs, lse, lod)"""
    return _solve_rhs_class().apply(rhs, lse, lod)
