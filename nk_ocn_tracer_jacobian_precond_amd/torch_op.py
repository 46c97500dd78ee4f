"""A differentiable solve for torch: X = A(val)^-1 B with gradients for B and for the matrix values.

The backward pass through a solve is a solve with A^T: with G = dL/dX,

    Lambda = A^-T G,      dL/dB = Lambda,      dL/dval[e] = - sum_c Lambda[c, row of e] * X[c, colind[e]]

(nkp_transpose for the first, nkp_value_gradient for the last; include/nkp.h).  The forward mode (torch.autograd.forward_ad dual
tensors) is the tangent solve nkp_solve_tangent_device: with the tangents dB and dval,

    dX = A^-1 (dB - dA X),      dA = dval on the pattern of A

torch is imported when NkpTorchSolver is constructed, not when this module is: the package stays importable without it.
"""
from __future__ import annotations

from . import solver as _solver

MAX_RHS = 8


class NkpTorchSolver:
    """Wraps an existing single-GPU NkpSolver.

        ts = NkpTorchSolver(solver)
        ts.set_values(val)            # CUDA float64 tensor, nnz entries in the solver's CSR order (may require grad)
        X = ts.solve(B)               # B: CUDA float64 (K, n), contiguous, K <= 8
        X.mul(W).sum().backward()     # B.grad = A^-T W, val.grad = the value gradient

    Streams: the constructor puts the solver (and with it its transposed solver) on torch's current stream,
    set_stream(torch.cuda.current_stream().cuda_stream), so the library's kernels are ordered with the caller's own and no
    extra synchronisation is needed.  Use the wrapper under the stream it was constructed under.

    The backward pass calls transposed() once -- the handle is kept by the solver and follows set_values -- and runs one
    batched solve there.  Forward mode runs one product with dval on the pattern (only when val carries a tangent) and one batched
    solve on the solver itself.  A forward, backward or tangent solve that does not converge raises NkpError: no partial
    gradient or tangent is returned.  Double backward is not supported.
    """

    def __init__(self, solver):
        import torch
        if not isinstance(solver, _solver.NkpSolver) or getattr(solver, "_comm", None) is not None:
            raise TypeError("NkpTorchSolver wraps a single-GPU NkpSolver")
        self.torch = torch
        self.solver = solver
        self.values = None
        solver.set_stream(torch.cuda.current_stream().cuda_stream)
        self._fn = _make_function(torch)

    def _check(self, t, shape, what):
        torch = self.torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"{what} must be a contiguous CUDA float64 tensor of shape {shape}")

    def set_values(self, val):
        """New matrix values on the solver's pattern (refactor_device); val is remembered as the leaf the gradient flows to."""
        self._check(val, (self.solver.nnz,), "val")
        self.solver.refactor_device(val.data_ptr())
        self.values = val

    def solve(self, B):
        """X = A^-1 B for the K rows of B, differentiable with respect to B and to the tensor given to set_values."""
        if B.dim() != 2 or not 1 <= B.shape[0] <= MAX_RHS:
            raise ValueError(f"B must have shape (K, {self.solver.n}) with 1 <= K <= {MAX_RHS}")
        self._check(B, (B.shape[0], self.solver.n), "B")
        val = self.values if self.values is not None else self.torch.empty(0, dtype=self.torch.float64, device=B.device)
        return self._fn.apply(B, val, self)


def _make_function(torch):
    class _Solve(torch.autograd.Function):
        @staticmethod
        def forward(ctx, B, val, owner):
            s = owner.solver
            X = torch.empty_like(B)
            s.solve_batch_device(B.data_ptr(), X.data_ptr(), B.shape[0], s.n)      # raises NkpError unless every column converged
            ctx.owner = owner
            ctx.save_for_backward(X)
            ctx.save_for_forward(X)
            # an input without a tangent reaches jvp as None, not as zeros: a dual on B alone makes no product with the values
            # (backward has one output and runs only with a gradient for it, so it never sees None)
            ctx.set_materialize_grads(False)
            return X

        @staticmethod
        def jvp(ctx, dB, dval, _):
            if dB is None and dval is None:
                return None
            s = ctx.owner.solver
            (X,) = ctx.saved_tensors
            dB = None if dB is None else dB.contiguous()
            dval = None if dval is None else dval.contiguous()
            dX = torch.empty_like(X)
            s.solve_tangent_device(None if dval is None else dval.data_ptr(), X.data_ptr(), s.n, None if dB is None else dB.data_ptr(), dX.data_ptr(),
                                   X.shape[0], s.n)                 # raises NkpError unless every column converged
            return dX

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, G):
            s = ctx.owner.solver
            (X,) = ctx.saved_tensors
            G = G.contiguous()
            Lam = torch.empty_like(G)
            s.transposed().solve_batch_device(G.data_ptr(), Lam.data_ptr(), G.shape[0], s.n)
            grad_val = None
            if ctx.needs_input_grad[1]:
                grad_val = torch.empty(s.nnz, dtype=torch.float64, device=G.device)
                s.value_gradient_device(Lam.data_ptr(), X.data_ptr(), G.shape[0], s.n, grad_val.data_ptr(), alpha=-1.0)
            return (Lam if ctx.needs_input_grad[0] else None), grad_val, None

    return _Solve
