"""Worker for tests/test_gpu_torch_second_order.py: second derivatives through NkpTorchSolver.solve, in a process of its own (torch
brings its own HIP runtime along).

synthetic 40x46x20 matrix, K = 2: (hB, hval, hW) = grad (<P, gB> + <q, gval>) with (gB, gval) = grad (<W, X>, create_graph) against
        the same chain made directly from the library calls (bits), the calls one such product makes, a plain .backward () against
        the direct calls (bits, and no graph left), and a double backward whose inner solve cannot converge.
golden fixtures, K = 2: the same (hB, hval, hW) against torch's own double differentiation of torch.linalg.solve on the dense
        A (val) on the CPU, with the norms the bound is made of, all taken on the dense side.
One JSON file."""
import argparse
import collections
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
GRID = (40, 46, 20)


def bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return bool(a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    from conftest import GOLDEN_CASES, GoldenCase
    from nk_ocn_tracer_jacobian_precond_amd import solver, synth
    from nk_ocn_tracer_jacobian_precond_amd.torch_op import NkpTorchSolver

    torch.cuda.set_device(0)
    dev = lambda h: torch.from_numpy(np.ascontiguousarray(h)).cuda()
    host = lambda t: t.detach().cpu().numpy()
    res = {}

    def hessian_vector(ts, B, val, W, P, q):
        ts.set_values(val)
        X = ts.solve(B)
        gB, gval = torch.autograd.grad(X.mul(W).sum(), (B, val), create_graph=True)
        Phi = gB.mul(P).sum() + gval.mul(q).sum()
        return torch.autograd.grad(Phi, (B, val, W))

    # ---------------------------------------------------------------- the composition, bit for bit
    p = synth.generate(imt=GRID[0], jmt=GRID[1], km=GRID[2], adv="upwind3", hmix="isop", seed=2, u_scale=3.0, ah=4.0e6, isop_k33=True)
    n, nnz = p.flat_len, p.colind.size
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    rng = np.random.default_rng(191)
    K = 2
    Bh, Wh, Ph, qh = rng.standard_normal((K, n)), rng.standard_normal((K, n)), rng.standard_normal((K, n)), p.nzval * rng.standard_normal(nnz)
    s = solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, 1, col_i=ci, col_j=cj, rtol=1e-10, restart=60, max_iters=3000)
    ts = NkpTorchSolver(s)
    B, val, W = dev(Bh).requires_grad_(True), dev(p.nzval).requires_grad_(True), dev(Wh).requires_grad_(True)
    P, q = dev(Ph), dev(qh)
    ts.set_values(val)
    t = s.transposed()
    made = collections.Counter()

    def count(obj, name, key):
        f = getattr(obj, name)

        def g(*args, **kw):
            made[key] += 1
            return f(*args, **kw)
        setattr(obj, name, g)
    count(s, "solve_batch_device", "solves")
    count(t, "solve_batch_device", "transposed_solves")
    count(s, "value_gradient_device", "value_gradients")
    count(s, "values_product_device", "products")
    calls0 = s.get_int("values_product_trans_calls")
    hB, hval, hW = hessian_vector(ts, B, val, W, P, q)
    torch.cuda.synchronize()
    res["calls"] = dict(made, products_trans=s.get_int("values_product_trans_calls") - calls0)

    # the chain of the table in torch_op.py, made directly: a transposed solve, two products, a solve, a transposed solve, two gradients
    with torch.no_grad():
        new = lambda like: torch.empty_like(like)
        Bd, vd, Wd = B.detach(), val.detach(), W.detach()
        X, Lam, U, Xbar, M, Lam2 = (new(Bd) for _ in range(6))
        g1, g2 = torch.empty(nnz, dtype=torch.float64, device="cuda"), torch.empty(nnz, dtype=torch.float64, device="cuda")
        s.solve_batch_device(Bd.data_ptr(), X.data_ptr(), K, n)
        t.solve_batch_device(Wd.data_ptr(), Lam.data_ptr(), K, n)
        s.values_product_device(q.data_ptr(), X.data_ptr(), K, n, U.data_ptr(), n, alpha=-1.0)
        s.values_product_trans_device(q.data_ptr(), Lam.data_ptr(), K, n, Xbar.data_ptr(), n, alpha=-1.0)
        Lbar = P + U
        s.solve_batch_device(Lbar.data_ptr(), M.data_ptr(), K, n)
        t.solve_batch_device(Xbar.data_ptr(), Lam2.data_ptr(), K, n)
        s.value_gradient_device(Lam.data_ptr(), M.data_ptr(), K, n, g1.data_ptr(), alpha=-1.0)
        s.value_gradient_device(Lam2.data_ptr(), X.data_ptr(), K, n, g2.data_ptr(), alpha=-1.0)
        torch.cuda.synchronize()
        res["composition"] = dict(hB=bits(host(hB), host(Lam2)), hval=bits(host(hval), host(g1 + g2)), hW=bits(host(hW), host(M)),
                                  nonzero=bool(hB.abs().max() > 0 and hval.abs().max() > 0 and hW.abs().max() > 0))
        # a plain backward: the direct calls of the first order
        gv = torch.empty(nnz, dtype=torch.float64, device="cuda")
        s.value_gradient_device(Lam.data_ptr(), X.data_ptr(), K, n, gv.data_ptr(), alpha=-1.0)
    B1, v1 = dev(Bh).requires_grad_(True), dev(p.nzval).requires_grad_(True)
    ts.set_values(v1)
    before = dict(made)
    ts.solve(B1).mul(W.detach()).sum().backward()
    torch.cuda.synchronize()
    res["first_order"] = dict(B=bits(host(B1.grad), host(Lam)), val=bits(host(v1.grad), host(gv)), no_graph=B1.grad.grad_fn is None and v1.grad.grad_fn is None,
                              calls={k: made[k] - before.get(k, 0) for k in made})
    s.close()

    # ---------------------------------------------------------------- an inner solve of the double backward that cannot converge
    # B = 0 and W = 0: the forward solve and the first backward converge at once (X = 0, Lambda = 0); the second backward solves
    # A M = P, which two steps do not
    s2 = solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, 1, col_i=ci, col_j=cj, rtol=1e-14, restart=3, max_iters=2)
    ts2 = NkpTorchSolver(s2)
    Bz, vz, Wz = torch.zeros_like(B).requires_grad_(True), dev(p.nzval).requires_grad_(True), torch.zeros_like(B).requires_grad_(True)
    got = None
    try:
        got = hessian_vector(ts2, Bz, vz, Wz, P, q)
        res["not_converged_raises"] = False
    except solver.NkpError as exc:
        res["not_converged_raises"] = exc.code == solver.NKP_NOT_CONVERGED and got is None
    s2.close()

    # ---------------------------------------------------------------- the mathematics, against torch's autograd on the dense matrix
    res["dense"] = []
    for name in GOLDEN_CASES:
        g = GoldenCase(name)
        gi, gj = solver.column_coords(g.ind_i, g.ind_j, g.col_start, g.cnt)
        rng = np.random.default_rng(131)
        Bh, Wh, Ph = rng.standard_normal((2, g.n)), rng.standard_normal((2, g.n)), rng.standard_normal((2, g.n))
        qh = g.val * rng.standard_normal(g.val.size)
        with solver.NkpSolver(g.rowptr, g.colind, g.val, g.blk_start, g.cnt, col_i=gi, col_j=gj, rtol=1e-12, restart=150, max_iters=5000) as sg:
            tg = NkpTorchSolver(sg)
            out = hessian_vector(tg, dev(Bh).requires_grad_(True), dev(g.val).requires_grad_(True), dev(Wh).requires_grad_(True), dev(Ph), dev(qh))
            torch.cuda.synchronize()
            hB, hval, hW = (host(o) for o in out)
        # the dense side, float64 on the CPU
        row = np.repeat(np.arange(g.n, dtype=np.int64), np.diff(g.rowptr.astype(np.int64)))
        col = g.colind.astype(np.int64)
        assert np.unique(row * g.n + col).size == col.size                                # no repeated entry: the bound's norm of a gradient
        ri, cidx = torch.from_numpy(row), torch.from_numpy(col)
        Bt, vt, Wt = (torch.from_numpy(x.copy()).requires_grad_(True) for x in (Bh, g.val, Wh))
        Pt, qt = torch.from_numpy(Ph), torch.from_numpy(qh)
        At = torch.zeros(g.n, g.n, dtype=torch.float64).index_put((ri, cidx), vt)
        Xt = torch.linalg.solve(At, Bt.T).T
        gBt, gvt = torch.autograd.grad(Xt.mul(Wt).sum(), (Bt, vt), create_graph=True)
        dB, dval, dW = (x.numpy() for x in torch.autograd.grad(gBt.mul(Pt).sum() + gvt.mul(qt).sum(), (Bt, vt, Wt)))
        A = At.detach().numpy()
        Q = np.zeros((g.n, g.n))
        Q[row, col] = qh
        Ainv = np.linalg.inv(A)
        X, Lam = (Ainv @ Bh.T).T, (Ainv.T @ Wh.T).T
        M, Lam2 = (Ainv @ (Ph - (Q @ X.T).T).T).T, (Ainv.T @ (-(Q.T @ Lam.T).T).T).T
        hv = -(Lam[:, row] * M[:, col]).sum(0) - (Lam2[:, row] * X[:, col]).sum(0)
        nrm = np.linalg.norm
        res["dense"].append(dict(name=name, n=g.n,
                                 diff=dict(hB=float(nrm(hB - dB)), hval=float(nrm(hval - dval)), hW=float(nrm(hW - dW))),
                                 ref=dict(hB=float(nrm(dB)), hval=float(nrm(dval)), hW=float(nrm(dW))),
                                 # the closed forms against torch's double differentiation, on the dense side alone
                                 closed_form=dict(hB=float(nrm(Lam2 - dB) / nrm(dB)), hW=float(nrm(M - dW) / nrm(dW)), hval=float(nrm(hv - dval) / nrm(dval))),
                                 norm=dict(Ainv=float(nrm(Ainv, 2)), A=float(nrm(A, 2)), AinvQ=float(nrm(Ainv @ Q, 2)), QAinv=float(nrm(Q @ Ainv, 2)), X=float(nrm(X)),
                                           Lam=float(nrm(Lam)), M=float(nrm(M)), Lam2=float(nrm(Lam2)))))
    with open(a.out, "w") as fh:
        json.dump(res, fh)


if __name__ == "__main__":
    main()
