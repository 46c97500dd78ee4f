"""Worker of tests/test_dist_smooth_plan.py (CPU, gloo): the lists of the fine-level exchange (tuning dist_smooth_exchange) in
the host plan of nkp_create_dist, launched once per rank on latitude bands.

  --mode plan      every rank asks for the exchange at --rings: the lists per colour against the overlap rows computed here from
                   the global matrix, the grid positions and the partition; the exchange itself run over gloo on global row ids
  --mode off       rank 0 asks for 1, the others for 0 (--ask-all 0: nobody asks): every list must be empty on every rank
  --mode refuse    rank --bad-rank (-1: every rank) asks for --value (out of range): every rank must refuse
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LISTS = ("smooth_send_rows0", "smooth_send_rows1", "smooth_recv_rows0", "smooth_recv_rows1", "smooth_give0", "smooth_give1", "smooth_need0", "smooth_need1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--grid", default="40x46x20")
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--rings", type=int, default=1)
    ap.add_argument("--value", type=int, default=2)
    ap.add_argument("--bad-rank", type=int, default=-1)
    ap.add_argument("--ask-all", type=int, default=1)
    ap.add_argument("--dump", default="", help="rank 0 writes the case for tests/dist_smooth_plan_main.cpp here")
    a = ap.parse_args()
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from nk_ocn_tracer_jacobian_precond_amd import dist as nd
    from nk_ocn_tracer_jacobian_precond_amd import solver, synth
    from dist_rings_worker import ring_sets

    imt, jmt, km = (int(t) for t in a.grid.split("x"))
    p = synth.generate(imt=imt, jmt=jmt, km=km, adv="upwind3", hmix="isop", seed=a.seed)
    n = p.flat_len
    blk = np.asarray(solver.column_blocks(p.col_start(), p.tracer_state_len, 1), np.int64)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    ci, cj = np.asarray(ci), np.asarray(cj)
    starts = nd.snap_partition(blk, world)
    loc = nd.local_slice(p.rowptr, p.colind, p.nzval, blk, starts, rank, ci, cj)
    f, m = int(loc["fst_row"]), int(loc["m_loc"])
    comm = nd.TorchComm()
    res = dict(rank=rank, fst=f, m_loc=m)

    if a.mode == "refuse":
        bad = a.bad_rank < 0 or rank == a.bad_rank
        try:
            nd.overlap_plan_host(loc, n, comm, 1, tuning=dict(dist_smooth_exchange=a.value if bad else 1))
            res["code"], res["message"] = 0, ""
        except solver.NkpError as exc:
            res["code"], res["message"] = exc.code, str(exc)
        res["bad"] = bool(bad)
    elif a.mode == "off":
        ask = 1 if (rank == 0 and a.ask_all) else 0
        pl = nd.overlap_plan_host(loc, n, comm, 1, tuning=dict(dist_smooth_exchange=ask, dist_ras_rings=a.rings))
        res.update(asked=ask, ras=int(pl["ras"]), smooth_exchange=int(pl["smooth_exchange"]), sizes={k: int(pl[k].size) for k in LISTS})
    else:
        import scipy.sparse as sp
        pl = nd.overlap_plan_host(loc, n, comm, 1, tuning=dict(dist_smooth_exchange=1, dist_ras_rings=a.rings))
        res.update(ras=int(pl["ras"]), ras_rings=int(pl["ras_rings"]), smooth_exchange=int(pl["smooth_exchange"]), n_sel=int(pl["n_sel"]))
        A = sp.csr_matrix((p.nzval, p.colind, p.rowptr), shape=(n, n))
        col_of = np.repeat(np.arange(blk.size - 1), np.diff(blk))
        rings = ring_sets(A, col_of, blk, ci, cj, f, m, a.rings)
        ov_cols = np.sort(np.concatenate(rings)) if rings else np.zeros(0, np.int64)
        ov_rows = np.concatenate([np.arange(blk[c], blk[c + 1]) for c in ov_cols]) if ov_cols.size else np.zeros(0, np.int64)
        ov_colour = (ci[col_of[ov_rows]] + cj[col_of[ov_rows]]) % 2
        owners = np.searchsorted(starts, ov_rows, side="right") - 1
        res["n_sel_expected"] = int(ov_rows.size)
        res["ring_cols"] = [int(r.size) for r in rings]
        own_colour = (ci[col_of[f:f + m]] + cj[col_of[f:f + m]]) % 2
        for c in (0, 1):
            send, recv, give, need = pl[f"smooth_send_rows{c}"].astype(np.int64), pl[f"smooth_recv_rows{c}"].astype(np.int64), pl[f"smooth_give{c}"], pl[f"smooth_need{c}"]
            want = ov_rows[ov_colour == c]                     # hierarchy order = ascending global rows
            # the rows this rank expects: its overlap rows of colour c, each once, in hierarchy order (rows of the hierarchy's
            # matrix are [own | overlap rows ascending])
            res[f"recv_rows_ok{c}"] = bool(np.array_equal(recv, m + np.flatnonzero(ov_colour == c)))
            res[f"need_ok{c}"] = bool(need.size == world and np.array_equal(need, np.bincount(owners[ov_colour == c], minlength=world)))
            res[f"send_own_ok{c}"] = bool(send.size == give.sum() and (send >= 0).all() and (send < m).all() and (own_colour[send] == c).all())
            off = np.concatenate([[0], np.cumsum(give)])
            res[f"send_sorted_ok{c}"] = bool(all((np.diff(send[off[q]:off[q + 1]]) > 0).all() for q in range(world)))
            res[f"give{c}"], res[f"need{c}"] = give.tolist(), need.tolist()
            res[f"sent{c}"] = [(f + send[off[q]:off[q + 1]]).tolist() for q in range(world)]          # global ids, per destination
            noff = np.concatenate([[0], np.cumsum(need)])
            res[f"expected{c}"] = [want[noff[q]:noff[q + 1]].tolist() for q in range(world)] if need.sum() == want.size else None
            # ... and the exchange itself delivers them
            sbuf = torch.from_numpy((f + send).astype(np.float64))
            rbuf = torch.full((int(need.sum()),), -1.0, dtype=torch.float64)
            comm._exchange_host(sbuf, give.tolist(), rbuf, need.tolist())
            res[f"exchange_ok{c}"] = bool(np.array_equal(rbuf.numpy(), want.astype(np.float64)))
        res["lists"] = {k: pl[k].tolist() for k in LISTS}
        if a.dump and rank == 0:
            with open(a.dump, "w") as fh:
                fh.write(f"{world} {n} {blk.size - 1} {a.rings}\n")
                for arr in (starts, p.rowptr, p.colind, blk, ci, cj):
                    fh.write(" ".join(str(int(v)) for v in arr) + "\n")
                fh.write(" ".join(float(v).hex() for v in p.nzval) + "\n")
    with open(f"{a.out}.{rank}", "w") as fh:
        json.dump(res, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
