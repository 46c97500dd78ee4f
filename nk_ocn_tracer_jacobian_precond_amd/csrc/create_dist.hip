// The row-distributed flavour: nkp_create_dist (its host-side plan: dist_plan.cpp; the rank-local solver: create.hip) and
// nkp_gather_root.
#include "solver_impl.h"

#include <string.h>

#include <vector>

extern "C" int nkp_create_dist (nkp_solver **out, const nkp_options *opt, int64_t n_global, int64_t fst_row, int64_t m_loc,
                                int64_t nnz_loc, const int32_t *rowptr_loc, const int32_t *colind_glob, const double *val,
                                const int32_t *blk_start_loc, int64_t nblk_loc, int coupled_tracer_cnt, const nkp_comm_ops *comm)
{
   if (!out) return fail (NKP_EINVAL, "nkp_create_dist: out is NULL");
   *out = nullptr;
   nkp_tuning tune;
   {
      // a dist_ras_rings out of range is refused by every rank together (dist_plan) when there are peers to tell
      bool range_error = false;
      const int trc = resolve_tuning (opt, &tune, &range_error);
      if (trc && !(range_error && comm && comm->nranks > 1)) return trc;
   }
   if (!comm || (comm->nranks <= 1 && !tune.force_dist)) {
      if (fst_row != 0 || m_loc != n_global) return fail (NKP_EINVAL, "nkp_create_dist: a single rank must own all rows");
      return create_impl (out, opt, n_global, nnz_loc, rowptr_loc, colind_glob, val, blk_start_loc, nblk_loc, coupled_tracer_cnt, nullptr);
   }
   if (!comm->allreduce || !comm->alltoallv || !comm->alltoallv_i32_host || !comm->allgather_i64_host)
      return fail (NKP_EINVAL, "nkp_create_dist: incomplete nkp_comm_ops");
   if (!rowptr_loc || m_loc < 0 || nnz_loc < 0 || (nnz_loc > 0 && (!colind_glob || !val))) return fail (NKP_EINVAL, "nkp_create_dist: bad matrix arguments");
   const int P = comm->nranks, rank = comm->rank;
   std::vector<int64_t> starts (P + 1, 0);
   if (comm->allgather_i64_host (comm->ctx, fst_row, starts.data ())) return fail (NKP_ECOMM, "nkp_create_dist: allgather failed");
   starts[P] = n_global;
   for (int p = 0; p < P; p++)
      if (starts[p + 1] < starts[p] || starts[0] != 0) return fail (NKP_EINVAL, "nkp_create_dist: row blocks must be contiguous and ascending over the ranks");
   // (whether m_loc matches the next rank's fst_row is a per-rank finding: dist_plan checks it and all ranks leave together)

   nkp_options o;
   if (opt) o = *opt;
   else nkp_default_options (&o);
   o.rank = rank;
   o.tuning = &tune;               // resolved once for the plan and the create call below
   DistPlan D;
   int rc = dist_plan (D, comm, o, starts, fst_row, m_loc, nnz_loc, rowptr_loc, colind_glob, val, blk_start_loc, nblk_loc, coupled_tracer_cnt);
   if (rc) return rc;
   // diagonal block: what the create path validates and what the hierarchy is built from without overlap
   std::vector<int32_t> drow ((size_t) m_loc + 1, 0), dcol;
   std::vector<double> dval;
   dcol.reserve ((size_t) nnz_loc);
   dval.reserve ((size_t) nnz_loc);
   for (int64_t r = 0; r < m_loc; r++) {
      for (int e = rowptr_loc[r]; e < rowptr_loc[r + 1]; e++)
         if (D.colind_ext[e] < m_loc) { dcol.push_back (D.colind_ext[e]); dval.push_back (val[e]); }
      drow[r + 1] = (int32_t) dcol.size ();
   }
   SpmvMatrixHost M = { nnz_loc, m_loc + D.n_halo, rowptr_loc, D.colind_ext.data (), val };
   PrecondMatrixHost PM = { m_loc + D.n_sel, (int64_t) D.e_blk.size () - 1, D.e_rowptr.data (), D.e_colind.data (), D.e_val.data (), D.e_blk.data (), D.e_ci.data (), D.e_cj.data (), D.e_ct.data () };
   nkp_solver *s = nullptr;
   rc = create_impl (&s, &o, m_loc, (int64_t) dcol.size (), drow.data (), dcol.data (), dval.data (), blk_start_loc, nblk_loc, coupled_tracer_cnt, &M, D.ras ? &PM : nullptr);
   // every rank must reach the collectives below even if its own setup failed: agree on success first
   {
      int64_t flag = rc ? 1 : 0;
      std::vector<int64_t> all (P + 1, 0);
      if (comm->allgather_i64_host (comm->ctx, flag, all.data ())) { if (s) solver_free (s); return fail (NKP_ECOMM, "nkp_create_dist: allgather failed"); }
      for (int p = 0; p < P; p++)
         if (all[p]) {
            if (s) solver_free (s);
            return rc ? rc : fail (NKP_ECOMM, "nkp_create_dist: setup failed on rank %d", p);
         }
   }
   s->dist.ops = *comm;
   s->dist.n_global = n_global;
   s->dist.fst = fst_row;
   s->dist.n_halo = D.n_halo;
   // the SpMV halo: its rows land behind the own rows of xe (K wide: of bxe), so it has no receive buffer
   bool ok = exchange_install (s, s->dist.x_halo, D.send_rows.data (), D.give, D.need, false, D.nsend, -1, -1) && dev_alloc (s, &s->dist.xe, (size_t) (m_loc + D.n_halo)) == NKP_OK;
   if (ok && D.ras) {
      s->dist.n_sel = D.n_sel;
      s->dist.n_ext = m_loc + D.n_sel;
      s->dist.ras_rings = D.rings;
      s->dist.ras_sep = D.rings >= 2;
      ok = dev_alloc (s, &s->dist.rext, (size_t) (m_loc + D.n_sel)) == NKP_OK && dev_alloc (s, &s->dist.zext, (size_t) (m_loc + D.n_sel)) == NKP_OK;
      if (!s->dist.ras_sep) {
         ok = ok && dev_alloc (s, &s->dist.sel_idx, (size_t) D.n_sel) == NKP_OK;
         if (ok && D.n_sel) ok = hipMemcpy (s->dist.sel_idx, D.sel_hpos.data (), (size_t) D.n_sel * sizeof (int), hipMemcpyHostToDevice) == hipSuccess;
      } else {
         // (one row wide the overlap rows arrive at rext + n, K wide in a buffer of the exchange)
         ok = ok && exchange_install (s, s->dist.x_ras, D.ras_send_rows.data (), D.ras_give, D.ras_need, false, (int64_t) D.ras_send_rows.size (), -1, D.n_sel);
      }
      s->dist.ras = ok;
   }
   // fine-level exchange (tuning dist_smooth_exchange, agreed by dist_plan): lists, counts, buffers; the index lists follow the
   // hierarchy.  A rank's cycle makes 4 nu - 1 exchanges, nu = its level-0 sweeps, so the exchange is only in force when level 0
   // of every rank runs the same nu half sweeps: each rank's count rides on the agreement below (0: its level 0 runs none)
   int64_t smooth_nu = 0;
   if (ok && D.ras && D.smooth) {
      ok = smooth_install (s, D);
      if (ok && ml_level0_hookable (s->ml)) {
         ok = smooth_build_lists (s) == 0;
         smooth_nu = ml_level0_sweeps (s->ml);
      }
   }
   {
      // once more all ranks together: a rank without halo buffers must not leave its peers to a first SpMV that never completes
      std::vector<int64_t> all (P + 1, 0);
      const bool comm_ok = comm->allgather_i64_host (comm->ctx, (ok ? 0 : 1) + 2 * smooth_nu, all.data ()) == 0;
      int bad_rank = -1;
      for (int p = 0; p < P && comm_ok; p++) if ((all[p] & 1) && bad_rank < 0) bad_rank = p;
      s->dist.smooth = comm_ok && smooth_nu > 0;
      for (int p = 0; p < P && comm_ok; p++) s->dist.smooth = s->dist.smooth && (all[p] >> 1) == smooth_nu;
      if (!ok || !comm_ok || bad_rank >= 0) {
         solver_free (s);
         if (!ok) return fail (NKP_ENOMEM, "nkp_create_dist: halo buffers could not be allocated");
         return fail (NKP_ECOMM, comm_ok ? "nkp_create_dist: halo buffers could not be allocated on rank %d" : "nkp_create_dist: allgather failed (%d)", bad_rank);
      }
   }
   {
      const bool want = s->tune.dist_overlap != 0;
      const int interior_blocks = s->dist.seg_rb[2] - s->dist.seg_rb[1];
      if (want && interior_blocks > 0 && hipStreamCreateWithFlags (&s->dist.comm_stream, hipStreamNonBlocking) == hipSuccess &&
          hipEventCreateWithFlags (&s->dist.ev_packed, hipEventDisableTiming) == hipSuccess &&
          hipEventCreateWithFlags (&s->dist.ev_halo, hipEventDisableTiming) == hipSuccess)
         s->dist.overlap = true;
   }
   s->dist.on = true;
   // nkp_transpose_dist builds A^T's row block from these and passes the caller's own block data to nkp_create_dist again
   s->dist.starts = starts;
   s->dist.h_halo_rows.assign (D.halo_rows.begin (), D.halo_rows.begin () + D.n_halo);
   s->dist.h_send_rows.assign (D.send_rows.begin (), D.send_rows.begin () + D.nsend);
   s->dist.own_has_blk = blk_start_loc != nullptr;
   if (blk_start_loc) s->dist.own_blk.assign (blk_start_loc, blk_start_loc + nblk_loc + 1);
   if (o.col_i) s->dist.own_ci.assign (o.col_i, o.col_i + nblk_loc);
   if (o.col_j) s->dist.own_cj.assign (o.col_j, o.col_j + nblk_loc);
   if (o.col_t) s->dist.own_ct.assign (o.col_t, o.col_t + nblk_loc);
   s->dist.own_tracer_cnt = coupled_tracer_cnt;
   if (s->opt.precond == NKP_PRECOND_MULTILEVEL) {
      // nkp_refactor_dist: the hierarchy's source matrix and where its values come from (host memory only until the first call)
      DistRefactorPlan *Q = new DistRefactorPlan;
      if (D.ras) {
         Q->n_src = m_loc + D.n_sel;
         Q->src_rowptr.swap (D.e_rowptr);
         Q->src_colind.swap (D.e_colind);
         Q->origin.swap (D.e_org);
         Q->ship.swap (D.ship_e);
         Q->ship_counts = D.ent_give;
         Q->recv_counts = D.ent_need;
         for (int c : Q->recv_counts) Q->n_recv += c;
         Q->exchange = true;
         // what a rebuild passes to ml_setup again (nkp_create's own copies are made for the diagonal block only)
         s->h_blk.swap (D.e_blk);
         s->h_col_i.swap (D.e_ci);
         s->h_col_j.swap (D.e_cj);
         s->h_col_t.swap (D.e_ct);
         s->tracer_cnt = coupled_tracer_cnt;
      } else {
         Q->n_src = m_loc;
         Q->origin.reserve (dcol.size ());
         for (int64_t e = 0; e < nnz_loc; e++)
            if (D.colind_ext[(size_t) e] < m_loc) Q->origin.push_back ((int32_t) e);
         Q->src_rowptr.swap (drow);
         Q->src_colind.swap (dcol);
      }
      Q->nnz_src = (int64_t) Q->src_colind.size ();
      s->dplan = Q;
   }
   msg (s, 1, "nkp_create_dist: %d of %d SpMV row blocks are interior (multiplied while the halo travels: %s)\n", s->dist.seg_rb[2] - s->dist.seg_rb[1],
        s->dist.seg_rb[3], s->dist.overlap ? "yes" : "no");
   msg (s, 1, "nkp_create_dist: rows [%lld, %lld) of %lld, %lld halo rows in, %lld rows out; overlap (restricted additive Schwarz): %s, %lld rows of other ranks in this rank's hierarchy (overlap depth %d)\n",
        (long long) fst_row, (long long) (fst_row + m_loc), (long long) n_global, (long long) D.n_halo, (long long) D.nsend, s->dist.ras ? "on" : "off", (long long) s->dist.n_sel,
        s->dist.ras ? s->dist.ras_rings : 0);
   if (D.smooth) msg (s, 1, "nkp_create_dist: fine-level exchange %s: %lld + %lld rows out, %lld + %lld rows in per pair of level-0 half sweeps\n", s->dist.smooth ? "on" : "agreed but not in force (the ranks' level-0 sweeps differ)",
                      (long long) D.smooth_send_rows[0].size (), (long long) D.smooth_send_rows[1].size (), (long long) D.smooth_recv_rows[0].size (), (long long) D.smooth_recv_rows[1].size ());
   *out = s;
   return NKP_OK;
}

extern "C" int nkp_gather_root (nkp_solver *s, const double *x_loc, double *x_global)
{
   if (!s || !x_loc) return fail (NKP_EINVAL, "nkp_gather_root: NULL argument");
   HIPCHK (hipSetDevice (s->device));
   if (!s->dist.on) {
      if (!x_global) return fail (NKP_EINVAL, "nkp_gather_root: NULL argument");
      memcpy (x_global, x_loc, (size_t) s->n * sizeof (double));
      return NKP_OK;
   }
   const int P = s->dist.ops.nranks, rank = s->dist.ops.rank;
   std::vector<int64_t> sizes (P + 1, 0);
   if (s->dist.ops.allgather_i64_host (s->dist.ops.ctx, s->n, sizes.data ())) return fail (NKP_ECOMM, "nkp_gather_root: allgather failed");
   std::vector<int> scnt (P, 0), rcnt (P, 0);
   scnt[0] = (int) s->n;                                  // everything goes to rank 0
   int64_t total = 0;
   if (rank == 0)
      for (int p = 0; p < P; p++) { rcnt[p] = (int) sizes[p]; total += sizes[p]; }
   double *dsend = s->t1, *drecv = nullptr;
   HIPCHK (hipMemcpyAsync (dsend, x_loc, (size_t) s->n * sizeof (double), hipMemcpyHostToDevice, s->stream));
   if (rank == 0) {
      if (!x_global) return fail (NKP_EINVAL, "nkp_gather_root: rank 0 needs x_global");
      HIPCHK (hipMalloc ((void **) &drecv, (size_t) (total ? total : 1) * sizeof (double)));
   }
   const int crc = s->dist.ops.alltoallv (s->dist.ops.ctx, dsend, scnt.data (), drecv ? (void *) drecv : (void *) s->t2, rcnt.data (), (void *) s->stream);
   if (!crc && rank == 0) {
      hipError_t e = hipMemcpyAsync (x_global, drecv, (size_t) total * sizeof (double), hipMemcpyDeviceToHost, s->stream);
      if (e != hipSuccess) { (void) hipFree (drecv); return fail (NKP_EDEVICE, "nkp_gather_root: copy back failed"); }
   }
   HIPCHK (hipStreamSynchronize (s->stream));
   if (drecv) (void) hipFree (drecv);
   return crc ? fail (NKP_ECOMM, "nkp_gather_root: exchange failed") : NKP_OK;
}
