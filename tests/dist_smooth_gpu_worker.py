"""Worker of tests/test_gpu_dist_smooth.py, one process per rank, all ranks on the test box's one GPU, collectives over the
library's file transport.  Latitude bands of the 40x46x20 problem (upwind3 + isop, seed 5).  All ranks run the same cases in the
same order (the calls are collective).  The knob is tuning dist_smooth_exchange.

  sweep      one cycle without coarse correction (ml_omega = 1e-300), knob on and off, against the same cycle of a single-GPU
             solver of the whole matrix: one ring, two rings, and the two-kernel half sweeps (ml_wave_fused = ml_lane_fused = 0)
  solve      knob off / on: iterations, relres re-checked on the host, counters of one cycle and of the solve
  batch      knob on: nkp_solve with nrhs = 4 against the same solver's single solves, bits and counters; once with precond_steps = 2
  refactor   knob on: nkp_refactor_dist_device (kept and rebuilt) against a fresh nkp_create_dist of the new values
  transpose  knob on: nkp_transpose_dist inherits the exchange and solves
  agree      rank 0 asks for 1, the others for 0; the field unset; an explicit 0
"""
import argparse
import ctypes as C
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

COUNTERS = ("dist_alltoallv_calls", "dist_allreduce_calls", "batch_steps", "batch_width")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", required=True)
    ap.add_argument("--file-dir", required=True)
    ap.add_argument("--grid", default="40x46x20")
    a = ap.parse_args()
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import oracle_binding as ora
    from nk_ocn_tracer_jacobian_precond_amd import dist as nd
    from nk_ocn_tracer_jacobian_precond_amd import solver, synth
    torch.cuda.set_device(0)
    lib = solver.load_library()

    imt, jmt, km = (int(t) for t in a.grid.split("x"))
    p = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=5)
    q = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=5, day_cnt=180.0)     # new values, same pattern
    n = p.flat_len
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    starts = nd.snap_partition(blk, world)
    loc = nd.local_slice(p.rowptr, p.colind, p.nzval, blk, starts, rank, ci, cj)
    loc_q = nd.local_slice(q.rowptr, q.colind, q.nzval, blk, starts, rank, ci, cj)
    f, m = int(loc["fst_row"]), int(loc["m_loc"])
    Bg = np.random.default_rng(11).standard_normal((4, n))
    Bg[2] *= 1e-3
    B = np.ascontiguousarray(Bg[:, f:f + m])

    lib.nkp_comm_file_init.argtypes = [C.POINTER(solver.NkpCommOps), C.c_char_p, C.c_int, C.c_int]
    lib.nkp_comm_file_free.argtypes = [C.POINTER(solver.NkpCommOps)]
    lib.nkp_comm_file_free.restype = None
    ops = solver.NkpCommOps()
    assert lib.nkp_comm_file_init(C.byref(ops), a.file_dir.encode(), rank, world) == 0
    comm = types.SimpleNamespace(ops=ops, errors=[])
    base = dict(rtol=1e-10, restart=60, max_iters=3000)
    # The exchange follows the half sweeps of level 0, so it is in force only where level 0 of EVERY rank's hierarchy is smoothed.
    # With the default ml_coarsest_rows = 8000 the smallest block of three bands of this grid (6943 own + 827 overlap rows) is one
    # dense level: no half sweeps there, and the ranks agree to leave the exchange out.  Every solver of these cases therefore
    # stops coarsening at 4000 rows instead (level 0 smoothed on every rank, one dense level below it), the single-GPU yardsticks
    # included; the "default" solves keep the default and report what is in force.
    SMOOTHED = dict(ml_coarsest_rows=4000)

    def make(tuning, lc=loc, smoothed=True, **options):
        tuning = dict(SMOOTHED if smoothed else {}, **(tuning or {}))
        return nd.NkpDistSolver(lc, n, comm, **dict(base, **options, tuning=tuning))

    def counters(s):
        return {k: s.get_int(k) for k in COUNTERS}

    def delta(after, before):
        return {k: after[k] - before[k] for k in COUNTERS[:3]}

    def checked_relres(s, x_loc, b_glob, prob):
        xg = np.zeros(n if rank == 0 else 1)
        rc = lib.nkp_gather_root(s._h, solver._p(np.ascontiguousarray(x_loc), C.c_double), solver._p(xg, C.c_double))
        assert rc == 0, lib.nkp_last_error().decode()
        if rank != 0:
            return None
        r = b_glob - ora.spmv(prob.rowptr, prob.colind, prob.nzval, xg)
        return float(np.linalg.norm(r) / np.linalg.norm(b_glob))

    res = dict(rank=rank, m_loc=m)
    cases = a.cases.split(",")
    if "sweep" in cases:
        out = {}
        rg = np.random.default_rng(7).standard_normal(n)
        for name, extra in (("ring1", {}), ("ring2", dict(dist_ras_rings=2)), ("two_kernel", dict(ml_wave_fused=0, ml_lane_fused=0))):
            tune = dict(SMOOTHED, ml_omega=1e-300, **extra)
            one = solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, 1, ci, cj, tuning=dict(tune), **base)
            zs = one.precond_apply(rg)[f:f + m]
            one.close()
            rec = dict(zs_max=float(np.abs(zs).max()))
            for knob in (1, 0):
                s = make(dict(tune, dist_smooth_exchange=knob))
                c0 = counters(s)
                zd = s.precond_apply(rg[f:f + m])
                rec["on" if knob else "off"] = dict(diff=float(np.abs(zd - zs).max()), in_force=s.get_int("dist_smooth_exchange"), rings=s.get_int("dist_ras_rings"),
                                                    ras_rows=s.get_int("dist_ras_rows"), smooth_rows=s.get_int("dist_smooth_rows"),
                                                    alltoallv=delta(counters(s), c0)["dist_alltoallv_calls"], levels=s.get_int("levels"))
                s.close()
            out[name] = rec
        res["sweep"] = out
    if "solve" in cases:
        out = {}
        for tname, smoothed in (("smoothed", True), ("default", False)):
            rec = {}
            if rank == 0:                                      # the undivided solve, for the record
                one = solver.NkpSolver(p.rowptr, p.colind, p.nzval, blk, 1, ci, cj, tuning=dict(SMOOTHED if smoothed else {}), **base)
                rec["single_iters"] = one.solve(Bg[0], raise_on_fail=False)[1]["iters"]
                one.close()
            for name, knob in (("off", 0), ("on", 1)):
                s = make(dict(dist_smooth_exchange=knob), smoothed=smoothed)
                c0 = counters(s)
                s.precond_apply(B[1])
                c1 = counters(s)
                x, info = s.solve(B[0], raise_on_fail=False)
                c2 = counters(s)
                rec[name] = dict(info, in_force=s.get_int("dist_smooth_exchange"), levels=s.get_int("levels"), apply_delta=delta(c1, c0), solve_delta=delta(c2, c1),
                                 device_bytes=s.get_int("device_bytes"), relres_checked=checked_relres(s, x, Bg[0], p))
                s.close()
            out[tname] = rec
        res["solve"] = out
    if "batch" in cases:
        out = {}
        for name, options in (("steps1", {}), ("steps2", dict(precond_steps=2))):
            s = make(dict(dist_smooth_exchange=1), **options)
            single = []
            for c in range(4):
                c0 = counters(s)
                x, info = s.solve(B[c], raise_on_fail=False)
                single.append(dict(x=x, info=info, delta=delta(counters(s), c0)))
            c0 = counters(s)
            X, infos = s.solve_many(B, raise_on_fail=False)
            c1 = counters(s)
            cols = [dict(x_equal=bool(np.array_equal(X[c], single[c]["x"])), iters=infos[c]["iters"], iters_single=single[c]["info"]["iters"],
                         relres_equal=bool(infos[c]["relres"] == single[c]["info"]["relres"]), berr_equal=bool(infos[c]["berr"] == single[c]["info"]["berr"]),
                         status=infos[c]["status"]) for c in range(4)]
            out[name] = dict(columns=cols, delta=delta(c1, c0), batch_width=c1["batch_width"], in_force=s.get_int("dist_smooth_exchange"),
                             single=[dict(o["info"], delta=o["delta"]) for o in single], equil=s.get_int("equil"), precond_steps=s.get_int("precond_steps"))
            s.close()
        res["batch"] = out
    if "refactor" in cases:
        out = {}
        on = dict(dist_smooth_exchange=1)
        for name, rebuild in (("kept", False), ("rebuild", True)):
            s = make(on)
            d = torch.from_numpy(np.ascontiguousarray(loc_q["val"])).cuda()
            torch.cuda.synchronize()
            s.refactor_dist_device(d.data_ptr(), rebuild=rebuild)
            del d
            t = make(on, loc_q)
            xs_, ins = s.solve(B[0], raise_on_fail=False)
            xt, int_ = t.solve(B[0], raise_on_fail=False)
            out[name] = dict(x_equal=bool(np.array_equal(xs_, xt)), iters=ins["iters"], iters_fresh=int_["iters"], relres=ins["relres"],
                             relres_fresh=int_["relres"], status=ins["status"], rebuilt=s.get_int("refactor_rebuilt"),
                             in_force=s.get_int("dist_smooth_exchange"), in_force_fresh=t.get_int("dist_smooth_exchange"))
            s.close()
            t.close()
        res["refactor"] = out
    if "transpose" in cases:
        s = make(dict(dist_smooth_exchange=1))
        t = s.transposed_dist()
        c0 = counters(t)
        t.precond_apply(B[1])
        c1 = counters(t)
        x, info = t.solve(B[0], raise_on_fail=False)
        At = p.scipy_csr().T.tocsr()
        At.sort_indices()
        pt = types.SimpleNamespace(rowptr=At.indptr.astype(np.int32), colind=At.indices.astype(np.int32), nzval=At.data)
        res["transpose"] = dict(info, in_force=t.get_int("dist_smooth_exchange"), in_force_source=s.get_int("dist_smooth_exchange"),
                                is_transpose=t.get_int("is_transpose"), apply_alltoallv=delta(c1, c0)["dist_alltoallv_calls"],
                                relres_checked=checked_relres(t, x, Bg[0], pt))
        s.close()
    if "agree" in cases:
        out, xs = {}, {}
        for name, tuning in (("mixed", dict(dist_smooth_exchange=1 if rank == 0 else 0)), ("unset", {}), ("zero", dict(dist_smooth_exchange=0))):
            s = make(tuning)
            c0 = counters(s)
            x, info = s.solve(B[0], raise_on_fail=False)
            xs[name] = x
            out[name] = dict(info, in_force=s.get_int("dist_smooth_exchange"), alltoallv=delta(counters(s), c0)["dist_alltoallv_calls"])
            s.close()
        out["x_equal_mixed_unset"] = bool(np.array_equal(xs["mixed"], xs["unset"]))
        out["x_equal_zero_unset"] = bool(np.array_equal(xs["zero"], xs["unset"]))
        res["agree"] = out
    lib.nkp_comm_file_free(C.byref(comm.ops))
    with open(f"{a.out}.{rank}", "w") as fh:
        json.dump(res, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
