"""A differentiable solve for torch: X = A(val)^-1 B with gradients for B and for the matrix values.

The backward pass through a solve is a solve with A^T: with G = dL/dX,

    Lambda = A^-T G,      dL/dB = Lambda,      dL/dval[e] = - sum_c Lambda[c, row of e] * X[c, colind[e]]

(nkp_transpose for the first, nkp_value_gradient for the last; include/nkp.h).  The forward mode (torch.autograd.forward_ad dual
tensors) is the tangent solve nkp_solve_tangent_device: with the tangents dB and dval,

    dX = A^-1 (dB - dA X),      dA = dval on the pattern of A

Second and higher derivatives: the backward pass is itself written with differentiable operations.  With V the matrix that holds
values v on A's pattern, five operations are closed under differentiation -- the backward of each is made of the others:

    Solve (B, val) -> X                  backward: Lambda = SolveT (G, val); grad B = Lambda; grad val = ValueGradient (Lambda, X, -1)
    SolveT (G, val) -> Lambda            backward: M = Solve (Lbar, val); grad G = M; grad val = ValueGradient (Lambda, M, -1)
    ValueGradient (Lambda, X, a) -> g    backward: grad Lambda = ValuesProduct (gbar, X, a); grad X = ValuesProductT (gbar, Lambda, a)
    ValuesProduct (v, X, a) -> a V X     backward: grad v = ValueGradient (Ybar, X, a); grad X = ValuesProductT (v, Ybar, a)
    ValuesProductT (v, L, a) -> a V^T L  backward: grad v = ValueGradient (L, Ybar, a); grad L = ValuesProduct (v, Ybar, a)

(nkp_solve_batch_device on the solver and on its transposed handle, nkp_value_gradient_device, nkp_values_product_device,
nkp_values_product_trans_device).  torch's own graph does the rest.

torch is imported when NkpTorchSolver is constructed, not when this module is: the package stays importable without it.
"""
from __future__ import annotations

from types import SimpleNamespace

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
    extra synchronisation is needed.  Use the wrapper under the stream it was constructed under.  Side streams are covered by a
    test: tests/test_gpu_stream_order.py runs set_values, solve, backward, a Hessian-vector product and a forward-mode tangent
    under torch.cuda.stream(S) with every operand still being produced on S when the library is entered.

    The backward pass calls transposed() once -- the handle is kept by the solver and follows set_values -- and runs one
    batched solve there.  Forward mode runs one product with dval on the pattern (only when val carries a tangent) and one batched
    solve on the solver itself.  A forward, backward or tangent solve that does not converge raises NkpError: no partial
    gradient or tangent is returned.

    Second and higher derivatives are supported: torch.autograd.grad(..., create_graph=True) records the backward pass, and a
    Hessian-vector product (the gradient of <P, B.grad> + <q, val.grad>) then costs four batched solves in all -- the forward
    solve, the adjoint solve of the first backward, and one solve with A and one with A^T in the second -- plus products and
    value gradients on the pattern; the first product with the transposed pattern builds the solver's transposed index
    (nkp_values_product_trans).  Without create_graph the backward pass records nothing and costs what it did: one adjoint solve and
    one value gradient.  An inner solve that does not converge raises NkpError from the backward that needed it.  Differentiate
    again under the matrix values the forward solve saw: set_values between a solve and a backward through it changes the matrix
    every later solve of that backward uses.  Forward-over-reverse (dual tensors through a backward pass) is not supported.

    Row-distributed solvers are not wrapped here, but all five operations now exist on them (the fifth as
    NkpDistSolver.values_product_trans_dist*), so the same backward passes can be written over local slices.
    """

    def __init__(self, solver):
        import torch
        if not isinstance(solver, _solver.NkpSolver) or getattr(solver, "_comm", None) is not None:
            raise TypeError("NkpTorchSolver wraps a single-GPU NkpSolver")
        self.torch = torch
        self.solver = solver
        self.values = None
        self._controls = {}                  # what set_solve_controls was given, for a transposed handle that is made later
        solver.set_stream(torch.cuda.current_stream().cuda_stream)
        self._ops = _make_functions(torch)
        self._fn = self._ops.Solve

    def _check(self, t, shape, what):
        torch = self.torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"{what} must be a contiguous CUDA float64 tensor of shape {shape}")

    def set_values(self, val):
        """New matrix values on the solver's pattern (refactor_device); val is remembered as the leaf the gradient flows to."""
        self._check(val, (self.solver.nnz,), "val")
        self.solver.refactor_device(val.data_ptr())
        self.values = val

    def set_solve_controls(self, rtol=None, atol=None, max_iters=None):
        """nkp_set_solve_controls on the forward solver and on its transposed handle -- now when it exists, else once the first
        backward pass makes it -- so the solves of a backward pass run at the tolerance the driver chose for the forward ones.
        None leaves a value as it is on either handle."""
        self.solver.set_solve_controls(rtol, atol, max_iters)
        self._controls.update({k: v for k, v in (("rtol", rtol), ("atol", atol), ("max_iters", max_iters)) if v is not None})
        t = getattr(self.solver, "_trans", None)
        if t is not None:
            t.set_solve_controls(rtol, atol, max_iters)
            t._controls_seen = dict(self._controls)

    def get_solve_controls(self):
        """dict(forward=..., transposed=...) of NkpSolver.get_solve_controls; transposed is None while there is no such handle."""
        t = getattr(self.solver, "_trans", None)
        return dict(forward=self.solver.get_solve_controls(), transposed=None if t is None else t.get_solve_controls())

    def transposed(self):
        """the solver's transposed handle (made at the first call) at the controls this wrapper was given"""
        t = self.solver.transposed()
        if self._controls and getattr(t, "_controls_seen", None) != self._controls:
            t.set_solve_controls(**self._controls)
            t._controls_seen = dict(self._controls)
        return t

    def solve(self, B):
        """X = A^-1 B for the K rows of B, differentiable with respect to B and to the tensor given to set_values."""
        if B.dim() != 2 or not 1 <= B.shape[0] <= MAX_RHS:
            raise ValueError(f"B must have shape (K, {self.solver.n}) with 1 <= K <= {MAX_RHS}")
        self._check(B, (B.shape[0], self.solver.n), "B")
        val = self.values if self.values is not None else self.torch.empty(0, dtype=self.torch.float64, device=B.device)
        return self._fn.apply(B, val, self)


def _make_functions(torch):
    """The five operations of the module docstring.  Each has one output and takes `owner` (the NkpTorchSolver) last; alpha is a
    Python float.  A backward runs only the library calls whose result is asked for (needs_input_grad)."""

    def value_gradient(Lam, X, alpha, owner):
        return _ValueGradient.apply(Lam, X, alpha, owner)

    class _Solve(torch.autograd.Function):
        @staticmethod
        def forward(ctx, B, val, owner):
            s = owner.solver
            X = torch.empty_like(B)
            s.solve_batch_device(B.data_ptr(), X.data_ptr(), B.shape[0], s.n)      # raises NkpError unless every column converged
            ctx.owner = owner
            ctx.save_for_backward(X, val)
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
        def backward(ctx, G):
            # a forward that saved X alone (no values to differentiate again) still gets its first derivatives
            X, *rest = ctx.saved_tensors
            val = rest[0] if rest else X.new_empty(0)
            Lam = _SolveT.apply(G.contiguous(), val, ctx.owner)
            grad_val = value_gradient(Lam, X, -1.0, ctx.owner) if ctx.needs_input_grad[1] else None
            return (Lam if ctx.needs_input_grad[0] else None), grad_val, None

    class _SolveT(torch.autograd.Function):
        @staticmethod
        def forward(ctx, G, val, owner):
            s = owner.solver
            Lam = torch.empty_like(G)
            owner.transposed().solve_batch_device(G.data_ptr(), Lam.data_ptr(), G.shape[0], s.n)
            ctx.owner = owner
            ctx.save_for_backward(Lam, val)
            return Lam

        @staticmethod
        def backward(ctx, Lbar):
            Lam, val = ctx.saved_tensors
            M = _Solve.apply(Lbar.contiguous(), val, ctx.owner)
            grad_val = value_gradient(Lam, M, -1.0, ctx.owner) if ctx.needs_input_grad[1] else None
            return (M if ctx.needs_input_grad[0] else None), grad_val, None

    class _ValueGradient(torch.autograd.Function):
        @staticmethod
        def forward(ctx, Lam, X, alpha, owner):
            s = owner.solver
            Lam, X = Lam.contiguous(), X.contiguous()
            g = torch.empty(s.nnz, dtype=torch.float64, device=Lam.device)
            s.value_gradient_device(Lam.data_ptr(), X.data_ptr(), Lam.shape[0], s.n, g.data_ptr(), alpha=alpha)
            ctx.owner, ctx.alpha = owner, alpha
            ctx.save_for_backward(Lam, X)
            return g

        @staticmethod
        def backward(ctx, gbar):
            Lam, X = ctx.saved_tensors
            gbar = gbar.contiguous()
            grad_lam = _ValuesProduct.apply(gbar, X, ctx.alpha, ctx.owner) if ctx.needs_input_grad[0] else None
            grad_x = _ValuesProductT.apply(gbar, Lam, ctx.alpha, ctx.owner) if ctx.needs_input_grad[1] else None
            return grad_lam, grad_x, None, None

    class _ValuesProduct(torch.autograd.Function):
        @staticmethod
        def forward(ctx, v, X, alpha, owner):
            s = owner.solver
            v, X = v.contiguous(), X.contiguous()
            Y = torch.empty_like(X)
            s.values_product_device(v.data_ptr(), X.data_ptr(), X.shape[0], s.n, Y.data_ptr(), s.n, alpha=alpha, accumulate=False)
            ctx.owner, ctx.alpha = owner, alpha
            ctx.save_for_backward(v, X)
            return Y

        @staticmethod
        def backward(ctx, Ybar):
            v, X = ctx.saved_tensors
            Ybar = Ybar.contiguous()
            grad_v = value_gradient(Ybar, X, ctx.alpha, ctx.owner) if ctx.needs_input_grad[0] else None
            grad_x = _ValuesProductT.apply(v, Ybar, ctx.alpha, ctx.owner) if ctx.needs_input_grad[1] else None
            return grad_v, grad_x, None, None

    class _ValuesProductT(torch.autograd.Function):
        @staticmethod
        def forward(ctx, v, Lam, alpha, owner):
            s = owner.solver
            v, Lam = v.contiguous(), Lam.contiguous()
            Y = torch.empty_like(Lam)
            s.values_product_trans_device(v.data_ptr(), Lam.data_ptr(), Lam.shape[0], s.n, Y.data_ptr(), s.n, alpha=alpha, accumulate=False)
            ctx.owner, ctx.alpha = owner, alpha
            ctx.save_for_backward(v, Lam)
            return Y

        @staticmethod
        def backward(ctx, Ybar):
            v, Lam = ctx.saved_tensors
            Ybar = Ybar.contiguous()
            grad_v = value_gradient(Lam, Ybar, ctx.alpha, ctx.owner) if ctx.needs_input_grad[0] else None
            grad_lam = _ValuesProduct.apply(v, Ybar, ctx.alpha, ctx.owner) if ctx.needs_input_grad[1] else None
            return grad_v, grad_lam, None, None

    return SimpleNamespace(Solve=_Solve, SolveT=_SolveT, ValueGradient=_ValueGradient, ValuesProduct=_ValuesProduct, ValuesProductT=_ValuesProductT)
