"""Worker of tests/test_gpu_dist_rings.py, one process per rank, all ranks on the test box's one GPU, collectives over the
library's file transport.  Latitude bands of the 40x46x20 problem (upwind3 + isop, seed 5).  All ranks run the same cases
in the same order (the calls are collective).

  solve     depth unset / 1 / 2: iterations, relres re-checked on the host, solution bits, introspection
  batch     depth 1 and 2: nkp_solve with nrhs = 4 against the same solver's single solves, bits and counters
  refactor  depth 2: nkp_refactor_dist_device (and a forced rebuild) against a fresh nkp_create_dist of the new values
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

    def make(depth, lc=loc):
        over = {} if depth is None else dict(tuning=dict(dist_ras_rings=depth))
        return nd.NkpDistSolver(lc, n, comm, **dict(base, **over))

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
    if "solve" in cases:
        out, xs = {}, {}
        for name, depth in (("unset", None), ("1", 1), ("2", 2)):
            s = make(depth)
            x, info = s.solve(B[0], raise_on_fail=False)
            xs[name] = x
            out[name] = dict(info, rings=s.get_int("dist_ras_rings"), ras=s.get_int("dist_ras"), ras_rows=s.get_int("dist_ras_rows"),
                             device_bytes=s.get_int("device_bytes"), create_us=s.get_int("create_us"),
                             relres_checked=checked_relres(s, x, Bg[0], p))
            s.close()
        out["x_equal_unset_1"] = bool(np.array_equal(xs["unset"], xs["1"]))
        res["solve"] = out
    if "batch" in cases:
        out = {}
        for depth in (1, 2):
            s = make(depth)
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
            out[str(depth)] = dict(columns=cols, delta=delta(c1, c0), batch_width=c1["batch_width"], rings=s.get_int("dist_ras_rings"),
                                   single=[dict(o["info"], delta=o["delta"]) for o in single],
                                   equil=s.get_int("equil"), precond_steps=s.get_int("precond_steps"))
            s.close()
        res["batch"] = out
    if "refactor" in cases:
        out = {}
        for name, rebuild in (("kept", False), ("rebuild", True)):
            s = make(2)
            d = torch.from_numpy(np.ascontiguousarray(loc_q["val"])).cuda()
            torch.cuda.synchronize()
            s.refactor_dist_device(d.data_ptr(), rebuild=rebuild)
            del d
            t = make(2, loc_q)
            xs_, ins = s.solve(B[0], raise_on_fail=False)
            xt, int_ = t.solve(B[0], raise_on_fail=False)
            out[name] = dict(x_equal=bool(np.array_equal(xs_, xt)), iters=ins["iters"], iters_fresh=int_["iters"], relres=ins["relres"],
                             relres_fresh=int_["relres"], status=ins["status"], rebuilt=s.get_int("refactor_rebuilt"),
                             halo_values=s.get_int("refactor_halo_values"), rings=s.get_int("dist_ras_rings"), rings_fresh=t.get_int("dist_ras_rings"))
            s.close()
            t.close()
        res["refactor"] = out
    lib.nkp_comm_file_free(C.byref(comm.ops))
    with open(f"{a.out}.{rank}", "w") as fh:
        json.dump(res, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
