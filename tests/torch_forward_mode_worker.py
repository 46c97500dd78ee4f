"""Worker for tests/test_gpu_torch_forward_mode.py: NkpTorchSolver under torch.autograd.forward_ad, in a process of its own (torch
brings its own HIP runtime along).

synthetic 40x46x20 matrix: the tangent of ts.solve (B) with duals on B, on val and on both against solve_tangent_device on the same
        inputs (bits), the product counter, a tangent solve that does not converge, and .backward () with and
        without save_for_forward (bits).
golden fixtures, K = 2: <W, jvp (dB, dval)> against <B.grad, dB> + <val.grad, dval> and the figures of the bound.
One JSON file."""
import argparse
import json
import math
import os
import sys

import numpy as np
import scipy.sparse as sp

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
    import torch.autograd.forward_ad as fwAD
    from conftest import GOLDEN_CASES, GoldenCase
    from nk_ocn_tracer_jacobian_precond_amd import solver, synth
    from nk_ocn_tracer_jacobian_precond_amd.torch_op import NkpTorchSolver

    torch.cuda.set_device(0)
    dev = lambda h: torch.from_numpy(np.ascontiguousarray(h)).cuda()
    res = {}

    # ---------------------------------------------------------------- bits of the calls the forward mode is made of
    p = synth.generate(imt=GRID[0], jmt=GRID[1], km=GRID[2], adv="upwind3", hmix="isop", seed=2, u_scale=3.0, ah=4.0e6, isop_k33=True)
    n, nnz = p.flat_len, p.colind.size
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    rng = np.random.default_rng(91)
    K = 3
    B, dB, W = dev(rng.standard_normal((K, n))), dev(rng.standard_normal((K, n))), dev(rng.standard_normal((K, n)))
    val, dval = dev(p.nzval), dev(p.nzval * rng.standard_normal(nnz))
    s = solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, 1, col_i=ci, col_j=cj, rtol=1e-10, restart=60, max_iters=3000)
    ts = NkpTorchSolver(s)
    for name, tb, tv in (("dual_B", dB, None), ("dual_val", None, dval), ("dual_both", dB, dval)):
        calls, tang = s.get_int("values_product_calls"), s.get_int("tangent_calls")
        with fwAD.dual_level():
            ts.set_values(val if tv is None else fwAD.make_dual(val, tv))
            X, dX = fwAD.unpack_dual(ts.solve(B if tb is None else fwAD.make_dual(B, tb)))
            X, dX = X.clone(), None if dX is None else dX.clone()
        made = (s.get_int("values_product_calls") - calls, s.get_int("tangent_calls") - tang)
        direct = torch.empty_like(X)
        s.solve_tangent_device(None if tv is None else tv.data_ptr(), X.data_ptr(), n, None if tb is None else tb.data_ptr(), direct.data_ptr(), K, n)
        torch.cuda.synchronize()
        res[name] = dict(has_tangent=dX is not None, equal=dX is not None and bits(dX.cpu().numpy(), direct.cpu().numpy()), product_calls=made[0], tangent_calls=made[1])
    # no dual at all: no tangent, no tangent solve
    tang = s.get_int("tangent_calls")
    with fwAD.dual_level():
        ts.set_values(val)
        res["no_dual_no_tangent"] = fwAD.unpack_dual(ts.solve(B)).tangent is None and s.get_int("tangent_calls") == tang
    # .backward () with and without save_for_forward: the function of the parent commit, restated
    class Before(torch.autograd.Function):
        @staticmethod
        def forward(ctx, Bt, vt, owner):
            Xt = torch.empty_like(Bt)
            owner.solver.solve_batch_device(Bt.data_ptr(), Xt.data_ptr(), Bt.shape[0], owner.solver.n)
            ctx.owner = owner
            ctx.save_for_backward(Xt)                               # and no save_for_forward
            return Xt

        backward = ts._fn.backward

    grads = []
    for fn in (ts._fn, Before):
        Bg, vg = B.clone().requires_grad_(True), val.clone().requires_grad_(True)
        ts.set_values(vg)
        fn.apply(Bg, vg, ts).mul(W).sum().backward()
        torch.cuda.synchronize()
        grads.append((Bg.grad.cpu().numpy(), vg.grad.cpu().numpy()))
    res["backward_unchanged"] = bits(grads[0][0], grads[1][0]) and bits(grads[0][1], grads[1][1]) and bool(np.any(grads[0][1] != 0.0))
    s.close()

    # a tangent solve that does not converge raises: the forward solve of dB = 0 ... B = 0 converges at once, its tangent cannot in two steps
    s2 = solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, 1, col_i=ci, col_j=cj, rtol=1e-14, restart=3, max_iters=2)
    ts2 = NkpTorchSolver(s2)
    try:
        with fwAD.dual_level():
            ts2.solve(fwAD.make_dual(torch.zeros_like(B), dB))
        res["not_converged_raises"] = False
    except solver.NkpError as exc:
        res["not_converged_raises"] = exc.code == solver.NKP_NOT_CONVERGED
    s2.close()

    # a right-hand side with a NaN is not solved (nkp.h at nkp_solve): NkpError, and no tensor comes back
    s3 = solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, 1, col_i=ci, col_j=cj, rtol=1e-10, restart=60, max_iters=3000)
    Bn = B.clone()
    Bn[1, n // 2] = float("nan")
    got = None
    try:
        got = NkpTorchSolver(s3).solve(Bn)
        res["nan_row_raises"] = False
    except solver.NkpError as exc:
        res["nan_row_raises"] = exc.code == solver.NKP_BREAKDOWN and got is None and "holds a non-finite entry" in str(exc)
    s3.close()

    # ---------------------------------------------------------------- the two modes agree (golden fixtures, K = 2)
    res["consistency"] = []
    for name in GOLDEN_CASES:
        g = GoldenCase(name)
        gi, gj = solver.column_coords(g.ind_i, g.ind_j, g.col_start, g.cnt)
        rng = np.random.default_rng(31)
        Bh, Wh = rng.standard_normal((2, g.n)), rng.standard_normal((2, g.n))
        dBh, dvh = rng.standard_normal((2, g.n)), g.val * rng.standard_normal(g.val.size)
        with solver.NkpSolver(g.rowptr, g.colind, g.val, g.blk_start, g.cnt, col_i=gi, col_j=gj, rtol=1e-12, restart=150, max_iters=5000) as sg:
            tg = NkpTorchSolver(sg)
            Bt, vt, Wt = dev(Bh).requires_grad_(True), dev(g.val).requires_grad_(True), dev(Wh)
            tg.set_values(vt)
            Xt = tg.solve(Bt)
            Xt.mul(Wt).sum().backward()
            with fwAD.dual_level():
                tg.set_values(fwAD.make_dual(vt.detach(), dev(dvh)))
                dXt = fwAD.unpack_dual(tg.solve(fwAD.make_dual(Bt.detach(), dev(dBh)))).tangent.clone()
            torch.cuda.synchronize()
            Xh, dXh, Lh, gvh = Xt.detach().cpu().numpy(), dXt.cpu().numpy(), Bt.grad.cpu().numpy(), vt.grad.cpu().numpy()
        dA = sp.csr_matrix((dvh, g.colind, g.rowptr), shape=(g.n, g.n))
        R = np.stack([dBh[c] - dA @ Xh[c] for c in range(2)])
        forwards = math.fsum((Wh * dXh).ravel().tolist())
        backwards = math.fsum((Lh * dBh).ravel().tolist() + (gvh * dvh).tolist())
        norms = [[float(np.linalg.norm(v[c])) for c in range(2)] for v in (Wh, dXh, Lh, R)]
        res["consistency"].append(dict(name=name, forwards=forwards, backwards=backwards, norm_W=norms[0], norm_dX=norms[1], norm_Lam=norms[2], norm_R=norms[3]))
    with open(a.out, "w") as fh:
        json.dump(res, fh)


if __name__ == "__main__":
    main()
