"""Worker of tests/test_dist_rings.py (CPU, gloo): the host plan of nkp_create_dist with several rings of overlap
(tuning dist_ras_rings), launched once per rank.

  --mode plan      the plan at --rings against ring sets computed here from the global matrix, the column coordinates and
                   the partition; the residual exchange of the plan (ras_send_rows / ras_need / ras_give) run over gloo
  --mode hash      sha256 and size of every exported field of the plan and its scalars (compared with recorded plans)
  --mode mismatch  rank r asks for --rings + (r % 2) rings: every rank must end with the smallest depth
  --mode refuse    rank --bad-rank (-1: every rank) asks for --rings (out of range): every rank must refuse
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("colind_ext", "halo_rows", "send_rows", "need", "give", "rowptr", "colind", "val", "blk_start", "col_i", "col_j", "col_t", "sel_hpos")
# everything the plan exports: also the residual exchange of two or more rings and what nkp_refactor_dist redoes the values from
ALL_FIELDS = FIELDS + ("ras_send_rows", "ras_need", "ras_give", "origin", "ship", "ent_give", "ent_need")
SCALARS = ("ras", "n_sel", "n_halo", "ras_rings")


def ring_sets(A, col_of, gblk, gci, gcj, f, m, depth):
    """Ring k of the rank owning rows [f, f + m), by the definition: ring 1 = the lateral water columns of other ranks that own
    rows couple to; ring k + 1 = the lateral columns of other ranks, in no earlier ring, that rows of ring k couple to (lateral:
    (i, j) is not the position of an own column).  Returns a list of arrays of column ids, one per ring (empty rings cut off)."""
    own_cols = np.unique(col_of[f:f + m])
    own_pos = set(zip(np.asarray(gci)[own_cols].tolist(), np.asarray(gcj)[own_cols].tolist()))
    rings, seen = [], set()
    rows = np.arange(f, f + m)
    for _ in range(depth):
        ref = np.unique(A[rows].indices) if rows.size else np.zeros(0, np.int64)
        ref = ref[(ref < f) | (ref >= f + m)]
        cols = [int(c) for c in np.unique(col_of[ref]) if int(c) not in seen and (int(gci[c]), int(gcj[c])) not in own_pos]
        if not cols:
            break
        seen.update(cols)
        rings.append(np.asarray(cols, np.int64))
        rows = np.concatenate([np.arange(gblk[c], gblk[c + 1]) for c in cols])
    return rings


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--grid", default="40x46x20")
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--partition", default="bands")
    ap.add_argument("--rings", type=int, default=2, help="-9: leave the tuning unset (defaults + environment)")
    ap.add_argument("--bad-rank", type=int, default=-1)
    a = ap.parse_args()
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from nk_ocn_tracer_jacobian_precond_amd import dist as nd
    from nk_ocn_tracer_jacobian_precond_amd import solver, synth

    imt, jmt, km = (int(t) for t in a.grid.split("x"))
    p = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=a.seed)
    n = p.flat_len
    cnt = 1
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    gblk, gci, gcj = blk, ci, cj
    if a.partition == "tracers":
        loc, starts, n = nd.tracer_slice(p, rank, world)
        p = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=a.seed, coupled_tracer_cnt=world)
        gblk = solver.column_blocks(p.col_start(), p.tracer_state_len, world)
        gci, gcj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), world)
    elif a.partition == "cells":
        import types
        cnt = 2
        p2 = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=a.seed, coupled_tracer_cnt=cnt)
        blk2 = solver.column_blocks(p2.col_start(), p2.tracer_state_len, cnt)
        ci2, cj2 = solver.column_coords(p2.ind_i, p2.ind_j, p2.col_start(), cnt)
        loc, starts, perm = nd.cell_major_slice(p2.rowptr, p2.colind, p2.nzval, blk2, cnt, world, rank, ci2, cj2)
        n = p2.flat_len
        A2 = p2.scipy_csr()[perm][:, perm].tocsr()
        A2.sort_indices()
        p = types.SimpleNamespace(rowptr=A2.indptr.astype(np.int32), colind=A2.indices.astype(np.int32), nzval=A2.data)
        _, _, gblk, _, src = solver.cell_major_order(blk2, cnt)
        gci, gcj = np.asarray(ci2)[src], np.asarray(cj2)[src]
    else:
        starts = nd.snap_partition(blk, world)
        loc = nd.local_slice(p.rowptr, p.colind, p.nzval, blk, starts, rank, ci, cj)
    f, m = int(loc["fst_row"]), int(loc["m_loc"])
    comm = nd.TorchComm()
    res = dict(rank=rank, m_loc=m)
    tuning = None if a.rings == -9 else dict(dist_ras_rings=a.rings)

    if a.mode == "hash":
        pl = nd.overlap_plan_host(loc, n, comm, cnt) if tuning is None else nd.overlap_plan_host(loc, n, comm, cnt, tuning=tuning)
        res["ras"] = int(pl["ras"])
        res["sha256"] = {k: hashlib.sha256(np.ascontiguousarray(pl[k]).tobytes()).hexdigest() for k in ALL_FIELDS}
        res["sizes"] = {k: int(np.asarray(pl[k]).size) for k in ALL_FIELDS}
        res["scalars"] = {k: int(pl[k]) for k in SCALARS}
    elif a.mode == "refuse":
        bad = a.bad_rank < 0 or rank == a.bad_rank
        try:
            nd.overlap_plan_host(loc, n, comm, cnt, tuning=dict(dist_ras_rings=a.rings if bad else 2))
            res["code"], res["message"] = 0, ""
        except solver.NkpError as exc:
            res["code"], res["message"] = exc.code, str(exc)
        res["bad"] = bool(bad)
    else:
        import scipy.sparse as sp
        depth = a.rings + (rank % 2 if a.mode == "mismatch" else 0)
        pl = nd.overlap_plan_host(loc, n, comm, cnt, tuning=dict(dist_ras_rings=depth))
        agreed = a.rings if (a.mode != "mismatch" or world > 1) else depth
        res["asked"], res["ras_rings"], res["ras"], res["n_sel"] = depth, pl["ras_rings"], pl["ras"], int(pl["sel_hpos"].size)
        A = sp.csr_matrix((p.nzval, p.colind, p.rowptr), shape=(n, n))
        gblk = np.asarray(gblk, np.int64)
        col_of = np.repeat(np.arange(gblk.size - 1), np.diff(gblk))
        rings = ring_sets(A, col_of, gblk, gci, gcj, f, m, agreed)
        one = ring_sets(A, col_of, gblk, gci, gcj, f, m, 1)
        res["ring_cols"] = [int(r.size) for r in rings]
        res["ring1_cols"] = int(one[0].size) if one else 0
        ov_cols = np.sort(np.concatenate(rings)) if rings else np.zeros(0, np.int64)
        ov_rows = np.concatenate([np.arange(gblk[c], gblk[c + 1]) for c in ov_cols]) if ov_cols.size else np.zeros(0, np.int64)
        owners = np.searchsorted(starts, ov_rows, side="right") - 1
        res["reaches_non_adjacent"] = bool(np.any(np.abs(owners - rank) > 1))
        res["n_sel_expected"] = int(ov_rows.size)
        if pl["ras"]:
            own = np.arange(f, f + m)
            ext = np.concatenate([own, ov_rows])
            want = A[ext][:, ext].tocsr()
            want.sort_indices()
            res["ext_matrix_ok"] = bool(np.array_equal(pl["rowptr"], want.indptr) and np.array_equal(pl["colind"], want.indices)
                                        and np.array_equal(pl["val"], want.data))
            own_cols = np.unique(col_of[own])
            cols = np.concatenate([own_cols, ov_cols])
            res["blocks_ok"] = bool(np.array_equal(pl["blk_start"], np.concatenate([[0], np.cumsum(np.diff(gblk)[cols])])))
            res["coords_ok"] = bool(np.array_equal(pl["col_i"], np.asarray(gci)[cols]) and np.array_equal(pl["col_j"], np.asarray(gcj)[cols]))
            # sel_hpos: the halo position of every overlap row that the SpMV halo holds (ring 1), -1 for the others
            hp = pl["sel_hpos"]
            in_halo = hp >= 0
            res["sel_hpos_ok"] = bool(hp.size == ov_rows.size and np.array_equal(pl["halo_rows"][hp[in_halo]], ov_rows[in_halo])
                                      and (agreed < 2 or not np.isin(ov_rows[~in_halo], pl["halo_rows"]).any())
                                      and (agreed >= 2 or in_halo.all()))
            # the residual exchange of the plan delivers exactly the overlap rows, in the hierarchy's order
            res["ras_need"], res["ras_give"] = pl["ras_need"].tolist(), pl["ras_give"].tolist()
            if agreed >= 2:
                xg = np.random.default_rng(3).standard_normal(n)
                give, need = pl["ras_give"], pl["ras_need"]
                send = torch.from_numpy(xg[f + pl["ras_send_rows"].astype(np.int64)].copy())
                recv = torch.empty(int(need.sum()), dtype=torch.float64)
                comm._exchange_host(send, give.tolist(), recv, need.tolist())
                res["ras_exchange_ok"] = bool(pl["ras_send_rows"].size == give.sum() and np.array_equal(recv.numpy(), xg[ov_rows])
                                              and np.array_equal(need, np.bincount(owners, minlength=world)))
                res["plan_reaches_non_adjacent"] = bool(any(need[q] > 0 and abs(q - rank) > 1 for q in range(world)))
            else:
                res["ras_exchange_ok"] = bool(pl["ras_send_rows"].size == 0 and pl["ras_need"].size == 0 and pl["ras_give"].size == 0)
    with open(f"{a.out}.{rank}", "w") as fh:
        json.dump(res, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
