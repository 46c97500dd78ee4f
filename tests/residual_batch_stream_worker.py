"""Worker for tests/test_gpu_residual_batch.py::test_a_late_x_on_the_callers_stream (a process of its own: torch is in it).

The solver (ragged_dd of tests/spmv_shapes.py, no preconditioner) is given a caller's non-blocking stream S.  X is filled with NaN;
on S a sleep kernel, the copy of the true X and an event are enqueued, and nkp_residual_batch_device is called at once, without a
synchronisation.  A reader anywhere but in order on S reads NaN.  R is read back on a stream that is not ordered with S: it must be
complete when the call returns.  Expected are the bits of the same calls made before set_stream, with torch.cuda.synchronize ()
around them.  A call whose producer had already finished when the library was entered has tested nothing and is reported so."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

SLEEP_MS = 30.0          # what the delay is scaled to; what decides is the per-call flag


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def calibrate(torch, S):
    def timed(cycles):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(S):
            e0.record(S)
            torch.cuda._sleep(cycles)
            e1.record(S)
        S.synchronize()
        return e0.elapsed_time(e1)
    timed(1000)
    probe = timed(10_000_000)
    return max(1, int(10_000_000 * SLEEP_MS / probe))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    import spmv_shapes as sh
    from nk_ocn_tracer_jacobian_precond_amd import solver

    torch.cuda.set_device(0)
    s = sh.ragged_dd()
    n = s.n
    rng = np.random.default_rng(94)
    B = torch.from_numpy(rng.standard_normal((8, n))).cuda()
    X = torch.from_numpy(rng.standard_normal((8, n))).cuda()
    torch.cuda.synchronize()
    h = solver.NkpSolver(s.rowptr, s.colind, s.val, None, precond=solver.PRECOND_NONE, restart=4)

    def call(x, nrhs, R):
        return h.residual_batch_device(B.data_ptr(), n, x.data_ptr(), n, nrhs, R.data_ptr(), n)

    expected = {}
    for nrhs in (1, 3, 8):
        R = torch.full((nrhs, n), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        nums = call(X, nrhs, R)
        torch.cuda.synchronize()
        expected[nrhs] = (np.stack(nums), R.cpu().numpy())

    S, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    h.set_stream(S.cuda_stream)
    cycles = calibrate(torch, S)
    res = dict(n=n, sleep_cycles=cycles, calls=[])

    # the control: the same poison, sleep and copy on S; a clone on a stream that does not wait for S must see the NaN
    T = torch.full_like(X, float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        torch.cuda._sleep(cycles)
        T.copy_(X, non_blocking=True)
    with torch.cuda.stream(S2):
        c = T.clone()
    torch.cuda.synchronize()
    res["control_saw_nan"] = bool(torch.isnan(c).any().item())
    res["late_values_arrived"] = bool(torch.equal(T, X))

    for nrhs in (1, 3, 8):
        Xl = torch.full((nrhs, n), float("nan"), dtype=torch.float64, device="cuda")
        R = torch.full((nrhs, n), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            torch.cuda._sleep(cycles)
            Xl.copy_(X[:nrhs], non_blocking=True)
            E = torch.cuda.Event()
            E.record(S)
            unfinished = not E.query()                               # immediately before the library is entered
            nums = call(Xl, nrhs, R)
        with torch.cuda.stream(S2):                                  # not ordered with S, no synchronisation of torch's
            Rc = R.clone()
            S2.synchronize()
        got = Rc.cpu().numpy()
        torch.cuda.synchronize()
        want_nums, want_R = expected[nrhs]
        res["calls"].append(dict(nrhs=nrhs, unfinished_at_entry=bool(unfinished), numbers_equal=bool(np.array_equal(u64(np.stack(nums)), u64(want_nums))),
                                 residual_equal=bool(np.array_equal(u64(got), u64(want_R))), finite=bool(np.isfinite(np.stack(nums)).all())))
    h.close()
    with open(a.out, "w") as fh:
        json.dump(res, fh)


if __name__ == "__main__":
    main()
