"""Worker for tests/test_gpu_refactor_dist.py (launched once per rank; gloo + host staging, all ranks share the one GPU).

Every rank builds a distributed solver on its slice, calls nkp_refactor_dist with new values and compares the result with a
fresh nkp_create_dist of those values, bit for bit: every array of every hierarchy level, the solution slice and the
iteration count.  One JSON file per rank: {case: {...}}.

  --partition bands    latitude bands of one matrix (restricted additive Schwarz unless NKP_DIST_RAS=0)
  --partition tracers  one coupled tracer per rank (no overlap)
  --cases              comma-separated: same, device, mixed, rebuild, drift, refuse (bands); same (any partition)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ARRAYS = ("rowptr", "colind", "valf", "val", "cmap", "rptr", "ridx", "blk_start", "fac", "perm0", "coarse_inv")
GRID = (40, 46, 20)


def gen(synth, **kw):
    a = dict(adv="upwind3", hmix="isop", seed=2, u_scale=3.0, ah=4.0e6, isop_k33=True)
    a.update(kw)
    return synth.generate(imt=GRID[0], jmt=GRID[1], km=GRID[2], **a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--partition", default="bands")
    ap.add_argument("--cases", default="same")
    ap.add_argument("--precond", default="multilevel")
    a = ap.parse_args()
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from nk_ocn_tracer_jacobian_precond_amd import dist as nd
    from nk_ocn_tracer_jacobian_precond_amd import solver, synth

    torch.cuda.set_device(0)
    comm = nd.TorchComm()
    p = gen(synth, day_cnt=365.0)
    same = gen(synth, day_cnt=180.0)                  # the same coarse cells
    differ = gen(synth, vdc_bg=100.0)                 # cells differ
    n = p.flat_len
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    opts = dict(rtol=1e-10, restart=60, max_iters=3000)
    if a.precond == "column":
        opts["precond"] = solver.PRECOND_COLUMN_JACOBI
    multilevel = a.precond == "multilevel"

    if a.partition == "tracers":
        def slice_of(prob):
            loc, starts_, n_ = nd.tracer_slice(prob, rank, world)
            return loc
        loc0, starts, n = nd.tracer_slice(p, rank, world)
    else:
        starts = nd.snap_partition(blk, world)

        def slice_of(prob, vals=None):
            return nd.local_slice(prob.rowptr, prob.colind, prob.nzval if vals is None else vals, blk, starts, rank, ci, cj)
    f, m = int(starts[rank]), int(starts[rank + 1] - starts[rank])
    b_loc = np.random.default_rng(11).standard_normal(n)[f:f + m]
    results = dict(rank=rank)

    def make(loc):
        return nd.NkpDistSolver(loc, n, comm, **opts)

    def arrays(s):
        if not multilevel:
            return []
        return [{k: s.ml_level_array(l, k) for k in ARRAYS} for l in range(s.get_int("levels"))]

    def compare(s, t):
        """bit equality of the hierarchy arrays, the SpMV, the preconditioner and the solve (collective: same calls on every rank)"""
        out = dict(levels=s.get_int("levels"))
        ha, hb = arrays(s), arrays(t)
        diff = []
        if len(ha) != len(hb):
            diff.append("levels")
        for l, (x, y) in enumerate(zip(ha, hb)):
            for k in ARRAYS:
                if x[k].shape != y[k].shape or not np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)):
                    diff.append(f"{l}:{k}")
        out["hier_diff"] = diff
        out["spmv_equal"] = bool(np.array_equal(s.spmv(b_loc), t.spmv(b_loc)))
        out["precond_equal"] = bool(np.array_equal(s.precond_apply(b_loc), t.precond_apply(b_loc)))
        xs, ins = s.solve(b_loc, raise_on_fail=False)
        xt, int_ = t.solve(b_loc, raise_on_fail=False)
        out["x_equal"] = bool(np.array_equal(xs, xt))
        out.update(status=ins["status"], iters=ins["iters"], iters_fresh=int_["iters"], relres=ins["relres"])
        return out

    def counters(s):
        return dict(rebuilt=s.get_int("refactor_rebuilt"), count=s.get_int("refactor_count"), halo_values=s.get_int("refactor_halo_values"),
                    ras_rows=s.get_int("dist_ras_rows"), ras=s.get_int("dist_ras"), refactor_us=s.get_int("refactor_us"))

    def check(loc_old, loc_new, rebuild=False, device=False, before=None):
        s = make(loc_old)
        if before is not None:
            before.update({k: s.ml_level_array(0, k).copy() for k in ("val", "valf")})
        if device:
            d = torch.from_numpy(np.ascontiguousarray(loc_new["val"])).cuda()
            torch.cuda.synchronize()
            s.refactor_dist_device(d.data_ptr(), rebuild=rebuild)
            del d
        else:
            s.refactor_dist(loc_new["val"], rebuild=rebuild)
        out = counters(s)
        if before is not None:
            out["level0_changed"] = bool(any(not np.array_equal(before[k], s.ml_level_array(0, k)) for k in ("val", "valf")))
        t = make(loc_new)
        out.update(compare(s, t))
        s.close()
        t.close()
        return out

    cases = a.cases.split(",")
    loc_p = slice_of(p)
    loc_q = slice_of(same)
    if "same" in cases:
        results["same"] = check(loc_p, loc_q)
    if "device" in cases:
        results["device"] = check(loc_p, loc_q, device=True)
    if "mixed" in cases:
        # only rank 0 has new values: the others' overlap rows from rank 0 change all the same
        results["mixed"] = check(loc_p, loc_q if rank == 0 else loc_p, before={})
    if "rebuild" in cases:
        results["rebuild"] = check(loc_p, slice_of(differ), rebuild=True)
    if "drift" in cases:
        import scipy.sparse as sp
        pl = nd.overlap_plan_host(loc_p, n, comm, 1)
        ovl = np.asarray(pl["halo_rows"], np.int64)[np.asarray(pl["sel_hpos"], np.int64)]
        sets = [None] * world
        dist.all_gather_object(sets, (f, m, ovl.tolist()))
        S = [set(range(ff, ff + mm)) | set(o) for ff, mm, o in sets]
        A = sp.csr_matrix((p.nzval, p.colind, p.rowptr), shape=(n, n))
        colid = np.repeat(np.arange(len(blk) - 1), np.diff(blk))
        rows = np.repeat(np.arange(n), np.diff(p.rowptr))
        aji = np.asarray(A.T.tocsr()[rows, p.colind]).ravel()
        dropped = np.nonzero((colid[rows] != colid[p.colind]) & (p.nzval < 0) & (p.nzval <= aji))[0]
        f1, m1 = sets[1][0], sets[1][1]
        others = set().union(*[S[r] for r in range(world) if r != 1])
        # (1) an interior row of rank 1 that no other rank holds, coupled to a row of rank 1
        c1 = [e for e in dropped if f1 <= rows[e] < f1 + m1 and f1 <= p.colind[e] < f1 + m1 and rows[e] not in others]
        # (2) an overlap row of rank 1 owned by rank 0, coupled to a row rank 1 holds
        ovl1 = set(sets[1][2])
        c2 = [e for e in dropped if rows[e] in ovl1 and sets[0][0] <= rows[e] < sets[0][0] + sets[0][1] and int(p.colind[e]) in S[1]]
        for name, cand in (("drift_own", c1), ("drift_overlap", c2)):
            e = int(cand[len(cand) // 2])
            v = p.nzval.copy()
            v[e] = -v[e]                               # the coupling every twin that holds both rows dropped is now positive
            i, j = int(rows[e]), int(p.colind[e])
            out = check(loc_p, slice_of(p, v))
            out["candidates"] = len(cand)
            out["expect_rebuilt"] = int(i in S[rank] and j in S[rank])
            results[name] = out
    if "refuse" in cases:
        s = make(loc_p)
        x0, i0 = s.solve(b_loc, raise_on_fail=False)
        bad = loc_q["val"].copy()
        if rank == 1:
            r = 7
            rp, cl = loc_q["rowptr"], loc_q["colind"]
            k = rp[r] + int(np.nonzero(cl[rp[r]:rp[r + 1]] == f + r)[0][0])
            bad[k] = 0.0
        try:
            s.refactor_dist(bad)
            out = dict(code=0, message="")
        except solver.NkpError as exc:
            out = dict(code=exc.code, message=str(exc))
        x1, i1 = s.solve(b_loc, raise_on_fail=False)
        out.update(unchanged=bool(np.array_equal(x0, x1)) and i0["iters"] == i1["iters"], count=s.get_int("refactor_count"))
        # and a good call afterwards succeeds on every rank
        s.refactor_dist(loc_q["val"])
        t = make(loc_q)
        out["after"] = compare(s, t)
        s.close()
        t.close()
        results["refuse"] = out
    results["comm_errors"] = comm.errors
    with open(f"{a.out}.{rank}", "w") as fh:
        json.dump(results, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
