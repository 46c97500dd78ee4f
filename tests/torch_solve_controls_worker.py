"""Worker for tests/test_gpu_solve_controls.py: NkpTorchSolver.set_solve_controls, in a process of its own -- torch brings its own
HIP runtime along, and it is imported before the library is loaded, as in the other torch workers.  One JSON file."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    from nk_ocn_tracer_jacobian_precond_amd.torch_op import NkpTorchSolver
    from test_gpu_solve_controls import BASE, CONFIGS, make, problem

    torch.cuda.set_device(0)
    km, opts = CONFIGS["multilevel"]
    p, _, _, _, B = problem(km)
    res = dict(created=dict(rtol=BASE["rtol"], atol=BASE["atol"], max_iters=BASE["max_iters"]))
    with make(km, **opts) as s:
        ts = NkpTorchSolver(s)
        ts.set_solve_controls(rtol=1e-5, max_iters=77)
        res["before_backward"] = ts.get_solve_controls()
        # the backward pass makes the transposed handle: it runs at the values the driver chose
        Bt = torch.tensor(B[:2], dtype=torch.float64, device="cuda", requires_grad=True)
        ts.solve(Bt).sum().backward()
        torch.cuda.synchronize()
        res["after_backward"] = ts.get_solve_controls()
        grad = Bt.grad.cpu().numpy()
        with make(km, **dict(opts, rtol=1e-5, max_iters=77)) as r:
            lam, _ = r.transposed().solve_many(np.ones((2, p.flat_len)))
        with make(km, **opts) as r:
            lam_default, _ = r.transposed().solve_many(np.ones((2, p.flat_len)))
        res["grad_equal"] = bool(grad.tobytes() == lam.tobytes())
        res["grad_differs_from_default"] = bool(grad.tobytes() != lam_default.tobytes())
        # a handle that exists follows at once
        ts.set_solve_controls(atol=1e-20)
        res["after_second_set"] = ts.get_solve_controls()
        del ts, Bt
    with open(a.out, "w") as fh:
        json.dump(res, fh)


if __name__ == "__main__":
    main()
