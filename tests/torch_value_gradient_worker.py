"""Worker for tests/test_gpu_value_gradient.py: NkpTorchSolver on the synthetic 40x46x20 matrix, in a process of its own.

first:  set_values(val), X = solve(B), (X * W).sum().backward() -- B.grad must have the bits of the transposed batched solve of W,
        val.grad those of value_gradient_device(Lambda, X, alpha = -1) and of the numpy restatement of the formula.
second: the same after set_values with other values on the same pattern: the results follow the new matrix.
One JSON file: {first: {...}, second: {...}, ...}."""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GRID = (40, 46, 20)


def gen(synth, **kw):
    a = dict(adv="upwind3", hmix="isop", seed=2, u_scale=3.0, ah=4.0e6, isop_k33=True)
    a.update(kw)
    return synth.generate(imt=GRID[0], jmt=GRID[1], km=GRID[2], **a)


def restate(rowptr, colind, lam, x, alpha):
    rowptr = np.asarray(rowptr, np.int64)
    row_of = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    col = np.asarray(colind, np.int64)
    s = lam[0][row_of] * x[0][col]
    for c in range(1, lam.shape[0]):
        s = s + lam[c][row_of] * x[c][col]
    return alpha * s


def bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return bool(a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    from nk_ocn_tracer_jacobian_precond_amd import solver, synth
    from nk_ocn_tracer_jacobian_precond_amd.torch_op import NkpTorchSolver

    torch.cuda.set_device(0)
    p, q = gen(synth), gen(synth, vdc_bg=100.0)
    assert np.array_equal(p.rowptr, q.rowptr) and np.array_equal(p.colind, q.colind) and not np.array_equal(p.nzval, q.nzval)
    n, nnz = p.flat_len, p.colind.size
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    rng = np.random.default_rng(51)
    Bh, Wh = rng.standard_normal((2, n)), rng.standard_normal((2, n))
    res = dict(n=n, nnz=nnz)

    s = solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, 1, col_i=ci, col_j=cj, rtol=1e-10, restart=60, max_iters=3000)
    ts = NkpTorchSolver(s)
    W = torch.from_numpy(Wh).cuda()
    previous = None
    for step, values in (("first", p.nzval), ("second", q.nzval)):
        val = torch.from_numpy(np.ascontiguousarray(values)).cuda().requires_grad_(True)
        B = torch.from_numpy(Bh).cuda().requires_grad_(True)
        ts.set_values(val)
        X = ts.solve(B)
        X.mul(W).sum().backward()
        # the calls the backward pass is documented to be made of, again and directly
        Lam = torch.empty_like(W)
        s.transposed().solve_batch_device(W.data_ptr(), Lam.data_ptr(), 2, n)
        gv = torch.empty(nnz, dtype=torch.float64, device="cuda")
        s.value_gradient_device(Lam.data_ptr(), X.data_ptr(), 2, n, gv.data_ptr(), alpha=-1.0)
        torch.cuda.synchronize()
        Xh, Lh, gh = X.detach().cpu().numpy(), Lam.cpu().numpy(), val.grad.cpu().numpy()
        A = sp.csr_matrix((values, p.colind, p.rowptr), shape=(n, n))
        out = dict(grad_B_is_transposed_solve=bits(B.grad.cpu().numpy(), Lh), grad_val_is_value_gradient=bits(gh, gv.cpu().numpy()),
                   grad_val_is_formula=bits(gh, restate(p.rowptr, p.colind, Lh, Xh, -1.0)), grad_val_shape=list(val.grad.shape),
                   residual=float(max(np.linalg.norm(A @ Xh[c] - Bh[c]) / np.linalg.norm(Bh[c]) for c in range(2))))
        if previous is not None:
            out.update(x_changed=not bits(Xh, previous[0]), grad_val_changed=not bits(gh, previous[1]))
        previous = (Xh, gh)
        res[step] = out

    # values that do not require grad: no gradient is computed for them, B still gets its own
    val = torch.from_numpy(np.ascontiguousarray(p.nzval)).cuda()
    B = torch.from_numpy(Bh).cuda().requires_grad_(True)
    ts.set_values(val)
    ts.solve(B).mul(W).sum().backward()
    res["no_grad_for_values"] = val.grad is None and B.grad is not None
    s.close()

    # a forward solve that does not converge raises: no silent partial result
    s2 = solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, 1, col_i=ci, col_j=cj, rtol=1e-14, restart=3, max_iters=2)
    ts2 = NkpTorchSolver(s2)
    try:
        ts2.solve(torch.from_numpy(Bh).cuda().requires_grad_(True))
        res["not_converged_raises"] = False
    except solver.NkpError as exc:
        res["not_converged_raises"] = exc.code == solver.NKP_NOT_CONVERGED
    s2.close()
    with open(a.out, "w") as fh:
        json.dump(res, fh)


if __name__ == "__main__":
    main()
