"""Worker for tests/test_gpu_transpose_dist.py (launched once per rank; gloo + host staging, all ranks share the one GPU).

Every rank builds a distributed solver on its row block of A, asks it for nkp_transpose_dist and compares the handle with a
fresh nkp_create_dist of the same rows of the host transpose (scipy: csr_matrix(...).T.tocsr() + sort_indices()), bit for bit.
One JSON file per rank: {case: {...}}.

  --matrix     synth (40x46x20), random (n = 1003, three ranks), golden:<fixture name>
  --partition  bands (latitude bands of one matrix) or tracers (one coupled tracer per rank)
  --cases      comma-separated: compare, refactor, ownership (synth); exchange (random); direct (golden)
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ARRAYS = ("rowptr", "colind", "valf", "val", "cmap", "rptr", "ridx", "blk_start", "fac", "perm0", "coarse_inv")
GRID = (40, 46, 20)
RANDOM_N, RANDOM_STARTS = 1003, [0, 301, 655, 1003]


def gen(synth, **kw):
    a = dict(adv="upwind3", hmix="isop", seed=2, u_scale=3.0, ah=4.0e6, isop_k33=True)
    a.update(kw)
    return synth.generate(imt=GRID[0], jmt=GRID[1], km=GRID[2], **a)


def random_matrix():
    """The matrix of the exchange test, from a seed: unsymmetric, rows sorted and duplicate-free, lengths 1 ... 150; no entry
    with its row on rank 2 and its column on rank 0; column 650 in 700 rows; column 17 and row 400 empty."""
    n, st, rng = RANDOM_N, RANDOM_STARTS, np.random.default_rng(7)
    lengths = rng.choice([1, 2, 3, 7, 20, 33, 64, 65, 150], size=n)
    long_rows = set(rng.choice(np.setdiff1d(np.arange(n), [400]), size=700, replace=False).tolist())
    rows = []
    for r in range(n):
        if r == 400:
            rows.append(np.empty(0, np.int64))
            continue
        allowed = np.setdiff1d(np.arange(st[1] if r >= st[2] else 0, n), [17, 650])
        c = rng.choice(allowed, size=lengths[r], replace=False)
        if r in long_rows:
            c[0] = 650
        rows.append(np.sort(c))
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
    colind = np.concatenate(rows).astype(np.int32)
    return rowptr, colind, rng.standard_normal(colind.size)


def transpose(rowptr, colind, val, n):
    T = sp.csr_matrix((val, colind, rowptr), shape=(n, n)).T.tocsr()
    T.sort_indices()
    return T


def rows_of(rowptr, colind, val, f, e):
    lo, hi = int(rowptr[f]), int(rowptr[e])
    return (np.asarray(rowptr[f:e + 1], np.int64) - lo).astype(np.int32), np.ascontiguousarray(colind[lo:hi], np.int32), np.ascontiguousarray(val[lo:hi], np.float64)


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return bool(a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--matrix", default="synth")
    ap.add_argument("--partition", default="bands")
    ap.add_argument("--cases", default="compare")
    ap.add_argument("--precond", default="multilevel")
    ap.add_argument("--rings", type=int, default=0)
    a = ap.parse_args()
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from nk_ocn_tracer_jacobian_precond_amd import dist as nd
    from nk_ocn_tracer_jacobian_precond_amd import solver, synth

    torch.cuda.set_device(0)
    comm = nd.TorchComm()
    lib = solver.load_library()
    opts = dict(rtol=1e-10, restart=60, max_iters=3000)
    if a.precond == "column":
        opts["precond"] = solver.PRECOND_COLUMN_JACOBI
    elif a.precond == "none":
        opts["precond"] = solver.PRECOND_NONE
    if a.rings:
        opts["tuning"] = dict(dist_ras_rings=a.rings)
    multilevel = a.precond == "multilevel"
    values = {}                                           # name -> values on A's pattern

    # ---- the global matrix, the row partition and this rank's block data
    if a.matrix == "random":
        rowptr, colind, values["p"] = random_matrix()
        n, starts = RANDOM_N, np.asarray(RANDOM_STARTS, np.int64)
        f, e = int(starts[rank]), int(starts[rank + 1])
        base = dict(blk_start=np.arange(e - f + 1, dtype=np.int32), fst_row=f, m_loc=e - f)
    elif a.matrix.startswith("golden:"):
        from conftest import GoldenCase
        g = GoldenCase(a.matrix.split(":", 1)[1])
        rowptr, colind, values["p"], n = g.rowptr, g.colind, g.val, g.n
        ci, cj = solver.column_coords(g.ind_i, g.ind_j, g.col_start, g.cnt)
        starts = nd.snap_partition(g.blk_start, world)
        base = nd.local_slice(rowptr, colind, g.val, g.blk_start, starts, rank, ci, cj)
        opts.update(rtol=1e-12, restart=150, max_iters=5000)
    else:
        probs = dict(p=gen(synth, day_cnt=365.0), same=gen(synth, day_cnt=180.0), differ=gen(synth, vdc_bg=100.0))
        p = probs["p"]
        if a.partition == "tracers":
            base, starts, n = nd.tracer_slice(p, rank, world)
            parts = {k: [synth.tracer_rows(q, r, world) for r in range(world)] for k, q in probs.items()}
            rowptr = np.concatenate([[0]] + [np.asarray(rp[1:], np.int64) + sum(int(x[0][-1]) for x in parts["p"][:r]) for r, (rp, _, _) in enumerate(parts["p"])])
            colind = np.concatenate([c for _, c, _ in parts["p"]])
            for k in probs:
                values[k] = np.concatenate([v for _, _, v in parts[k]])
        else:
            rowptr, colind, n = p.rowptr, p.colind, p.flat_len
            for k, q in probs.items():
                assert np.array_equal(q.rowptr, rowptr) and np.array_equal(q.colind, colind)
                values[k] = q.nzval
            blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
            ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
            starts = nd.snap_partition(blk, world)
            base = nd.local_slice(rowptr, colind, p.nzval, blk, starts, rank, ci, cj)
    f, m = int(starts[rank]), int(starts[rank + 1] - starts[rank])
    assert (f, m) == (int(base["fst_row"]), int(base["m_loc"]))
    b_glob = np.random.default_rng(11).standard_normal(n)
    b_loc = b_glob[f:f + m]
    B_loc = np.stack([np.random.default_rng(21 + k).standard_normal(n)[f:f + m] for k in range(4)])
    results = dict(rank=rank)

    def block(rp, ci_, v):
        """this rank's rows of a global CSR with this rank's block data"""
        r, c, w = rows_of(rp, ci_, v, f, f + m)
        return dict(base, rowptr=r, colind=c, val=w)

    def forward(name="p"):
        return block(rowptr, colind, values[name])

    def reference(name="p"):
        """rows [f, f + m) of the host transpose: never the code under test"""
        T = transpose(rowptr, colind, values[name], n)
        return block(T.indptr, T.indices, T.data)

    def make(loc):
        return nd.NkpDistSolver(loc, n, comm, **opts)

    def arrays(s):
        if not multilevel:
            return []
        return [{k: s.ml_level_array(l, k) for k in ARRAYS} for l in range(s.get_int("levels"))]

    def compare(t, u):
        """bit equality of the matrix sizes, the halo, the hierarchy arrays, the SpMV, the preconditioner, one solve and a batch of 4
        (collective: the same calls on every rank)"""
        out = dict(levels=t.get_int("levels"))
        out["sizes_equal"] = all(t.get_int(k) == u.get_int(k) for k in ("n", "nnz", "dist_halo_rows", "dist_ras", "dist_ras_rows", "dist_ras_rings", "rowblocks", "dist_interior_rowblocks"))
        ha, hb = arrays(t), arrays(u)
        diff = []
        if len(ha) != len(hb):
            diff.append("levels")
        for l, (x, y) in enumerate(zip(ha, hb)):
            for k in ARRAYS:
                if x[k].shape != y[k].shape or not np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)):
                    diff.append(f"{l}:{k}")
        out["hier_diff"] = diff
        out["spmv_equal"] = bits(t.spmv(b_loc), u.spmv(b_loc))
        out["precond_equal"] = bits(t.precond_apply(b_loc), u.precond_apply(b_loc))
        xt, it = t.solve(b_loc, raise_on_fail=False)
        xu, iu = u.solve(b_loc, raise_on_fail=False)
        out["x_equal"] = bits(xt, xu)
        Xt, _ = t.solve_many(B_loc, raise_on_fail=False)
        Xu, _ = u.solve_many(B_loc, raise_on_fail=False)
        out["many_equal"] = bits(Xt, Xu)
        out.update(status=it["status"], iters=it["iters"], iters_fresh=iu["iters"], relres=it["relres"], ras=t.get_int("dist_ras"), ras_rows=t.get_int("dist_ras_rows"),
                   ras_rings=t.get_int("dist_ras_rings"))
        return out

    def against_fresh(t, name):
        u = make(reference(name))
        out = compare(t, u)
        u.close()
        return out

    def code_of(fn):
        try:
            fn()
            return dict(code=0, message="")
        except solver.NkpError as exc:
            return dict(code=exc.code, message=str(exc))

    cases = a.cases.split(",")
    if "exchange" in cases:
        A = sp.csr_matrix((values["p"], colind, rowptr), shape=(n, n))
        T = transpose(rowptr, colind, values["p"], n)
        owner = np.searchsorted(starts, np.arange(n), side="right") - 1
        er, ec = owner[np.repeat(np.arange(n), np.diff(rowptr))], owner[colind]
        cross = np.array([[int(np.sum((er == i) & (ec == j))) for j in range(world)] for i in range(world)])
        props = dict(empty_2_to_0=int(cross[2, 0]) == 0, some_0_to_2=int(cross[0, 2]) > 0, col650=int(np.diff(T.indptr)[650]), col17=int(np.diff(T.indptr)[17]),
                     row400=int(np.diff(rowptr)[400]), col650_ranks=sorted(set(owner[T.indices[T.indptr[650]:T.indptr[651]]].tolist())),
                     sorted_rows=bool(A.has_sorted_indices), lengths=[int(np.diff(rowptr).min()), int(np.diff(rowptr).max())],
                     unsymmetric=bool((abs(A - A.T)).nnz > 0))
        s = make(forward())
        t = s.transposed_dist()
        u = make(reference())
        out = dict(props=props, spmv_equal=True, rel_err=0.0)
        for k in range(2):
            x = np.random.default_rng(31 + k).standard_normal(n)
            y = t.spmv(x[f:f + m])
            out["spmv_equal"] = out["spmv_equal"] and bits(y, u.spmv(x[f:f + m]))
            ref = (T @ x)[f:f + m]
            out["rel_err"] = max(out["rel_err"], float(np.linalg.norm(y - ref) / np.linalg.norm(ref)))
        out.update(sent=s.get_int("trans_sent_entries"), recv=s.get_int("trans_recv_entries"), want_sent=int(cross[rank].sum() - cross[rank, rank]),
                   want_recv=int(cross[:, rank].sum() - cross[rank, rank]), from_rank=[int(cross[q, rank]) for q in range(world)],
                   sizes_equal=t.get_int("nnz") == u.get_int("nnz") == int(T.indptr[f + m] - T.indptr[f]) and t.get_int("dist_halo_rows") == u.get_int("dist_halo_rows"),
                   is_transpose=[s.get_int("is_transpose"), t.get_int("is_transpose"), u.get_int("is_transpose")],
                   trans_us=s.get_int("trans_us"), trans_kernel_us=s.get_int("trans_kernel_us"))
        u.close()
        s.close()
        results["exchange"] = out

    if "compare" in cases:
        s = make(forward())
        x0, i0 = s.solve(b_loc, raise_on_fail=False)
        bytes0 = s.get_int("device_bytes")
        t = s.transposed_dist()
        out = against_fresh(t, "p")
        x1, i1 = s.solve(b_loc, raise_on_fail=False)
        out.update(forward_unchanged=bits(x0, x1) and i0["iters"] == i1["iters"] and i0["relres"] == i1["relres"], forward_bytes_unchanged=s.get_int("device_bytes") == bytes0,
                   sent=s.get_int("trans_sent_entries"), recv=s.get_int("trans_recv_entries"), forward_ras=s.get_int("dist_ras"), forward_ras_rows=s.get_int("dist_ras_rows"),
                   forward_iters=i0["iters"], trans_bytes=s.get_int("trans_device_bytes"), same_handle=s.transposed_dist() is t)
        s.close()
        out["closed_with_owner"] = t._h.value is None
        results["compare"] = out

    if "refactor" in cases:
        s = make(forward())
        t = s.transposed_dist()
        steps = []
        for name, how in (("same", "host"), ("p", "device"), ("differ", "rebuild")):
            new = forward(name)["val"]
            if how == "device":
                d = torch.from_numpy(np.ascontiguousarray(new)).cuda()
                torch.cuda.synchronize()
                s.refactor_dist_device(d.data_ptr())
                del d
            else:
                s.refactor_dist(new, rebuild=how == "rebuild")
            out = against_fresh(t, name)
            out.update(how=how, still_attached=s.transposed_dist() is t, count=s.get_int("refactor_count"), count_t=t.get_int("refactor_count"),
                       rebuilt=s.get_int("refactor_rebuilt"), rebuilt_t=t.get_int("refactor_rebuilt"))
            steps.append(out)
        results["refactor"] = steps
        # a refused refactor (a zero diagonal on rank 1) touches neither solver
        xs0, is0 = s.solve(b_loc, raise_on_fail=False)
        xt0, it0 = t.solve(b_loc, raise_on_fail=False)
        bad = forward("same")
        bad["val"] = bad["val"].copy()
        if rank == 1 % world:
            r = 7
            rp, cl = bad["rowptr"], bad["colind"]
            bad["val"][rp[r] + int(np.nonzero(cl[rp[r]:rp[r + 1]] == f + r)[0][0])] = 0.0
        out = code_of(lambda: s.refactor_dist(bad["val"]))
        xs1, is1 = s.solve(b_loc, raise_on_fail=False)
        xt1, it1 = t.solve(b_loc, raise_on_fail=False)
        out.update(forward_unchanged=bits(xs0, xs1) and is0["iters"] == is1["iters"], transposed_unchanged=bits(xt0, xt1) and it0["iters"] == it1["iters"],
                   still_attached=s.transposed_dist() is t, count=s.get_int("refactor_count"), count_t=t.get_int("refactor_count"))
        results["refuse"] = out
        s.close()

    if "ownership" in cases:
        s = make(forward())
        out = dict(bytes_before=s.get_int("trans_device_bytes"), own_bytes=s.get_int("device_bytes"))
        t = s.transposed_dist()
        h = C.c_void_p()
        out.update(bytes_held=s.get_int("trans_device_bytes"), t_bytes=t.get_int("device_bytes"), t_nnz=t.nnz, same_object=s.transposed_dist() is t,
                   same_handle=lib.nkp_transpose_dist(s._h, C.byref(h)) == 0 and h.value == t._h.value, own_bytes_after=s.get_int("device_bytes"))
        # the refusals on the transposed handle, on rank 0 ALONE: a collective reached here would leave rank 0 waiting for good
        if rank == 0:
            calls = t.get_int("dist_alltoallv_calls"), s.get_int("dist_alltoallv_calls")
            v = np.ascontiguousarray(reference()["val"])
            pv = v.ctypes.data_as(C.POINTER(C.c_double))
            d = torch.from_numpy(v).cuda()
            torch.cuda.synchronize()
            lib.nkp_clone.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
            refused = dict(refactor_dist=lib.nkp_refactor_dist(t._h, pv, 0), refactor_dist_device=lib.nkp_refactor_dist_device(t._h, C.c_void_p(d.data_ptr()), 0),
                           refactor=lib.nkp_refactor(t._h, pv, 0), refactor_device=lib.nkp_refactor_device(t._h, C.c_void_p(d.data_ptr()), 0),
                           clone=lib.nkp_clone(t._h, C.byref(h)), set_stream=lib.nkp_set_stream(t._h, None), transpose=lib.nkp_transpose(t._h, C.byref(h)),
                           transpose_dist=lib.nkp_transpose_dist(t._h, C.byref(h)))
            del d
            out.update(refused=refused, no_collective=calls == (t.get_int("dist_alltoallv_calls"), s.get_int("dist_alltoallv_calls")) and not comm.errors)
        xt, _ = t.solve(b_loc, raise_on_fail=False)
        # one rank destroys its handle alone: the next call is refused on every rank and names it
        if rank == 1:
            t.close()
        out["uneven"] = code_of(s.transposed_dist)
        if rank != 1:
            out["kept"] = bool(t._h.value) and t.get_int("is_transpose") == 1 and s.get_int("trans_device_bytes") == out["bytes_held"]
            t.close()
        out.update(bytes_after_close=s.get_int("trans_device_bytes"), own_bytes_after_close=s.get_int("device_bytes"))
        t2 = s.transposed_dist()                              # all ranks hold none again: a new one is built
        xt2, _ = t2.solve(b_loc, raise_on_fail=False)
        out.update(rebuilt_new=t2 is not t and s.get_int("trans_device_bytes") > 0, rebuilt_solves_same=bits(xt, xt2))
        s.close()
        out["closed_with_owner"] = t2._h.value is None
        t2.close()                                            # a no-op, not a second free
        results["ownership"] = out

    if "direct" in cases:
        s = make(forward())
        t = s.transposed_dist()
        sol = {}
        for grp in g.groups():
            x, info = t.solve(g.rhs(grp)[f:f + m], raise_on_fail=False)
            sol[grp] = dict(x=x.tolist(), status=info["status"], iters=info["iters"], relres=info["relres"])
        s.close()
        results["direct"] = dict(first_row=f, groups=sol)

    results["comm_errors"] = comm.errors
    with open(f"{a.out}.{rank}", "w") as fh:
        json.dump(results, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
