// libnkp_hip, C ABI (include/nkp.h): the life of a solver object -- devices, destruction, messages, the stream it works on and
// the counters it answers with.  Creation is create.hip and create_dist.hip, the solves are krylov.hip and batch_solve.hip, new
// matrix values on an existing solver (nkp_refactor and its kin) refactor_api.hip; the solver object and the map of the units that
// work on it are solver_impl.h.
#include "solver_impl.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

extern "C" int nkp_device_count (void)
{
   int n = 0;
   if (hipGetDeviceCount (&n) != hipSuccess) return 0;
   return n;
}

// ---------------------------------------------------------------- solver object
void solver_free (nkp_solver *s)
{
   if (!s) return;
   if (s->borrowed) {           // a clone owns its work vectors, its level vectors and its stream, nothing else
      void *own[] = { s->V, s->vcur, s->Z, s->w, s->r, s->x, s->b, s->t1, s->t2, s->p1, s->p2, s->eqtmp, s->partial, s->dscal, s->dint };
      for (void *p : own)
         if (p) (void) hipFree (p);
      for (MlLevel &L : s->ml.lev) {
         void *lv[] = { L.one.x, L.one.x2, L.one.b, L.one.r };
         for (void *p : lv)
            if (p) (void) hipFree (p);
      }
      valgrad_release (s);
      valprod_release (s);
      residual_release (s);
      if (s->hpin) (void) hipHostFree (s->hpin);
      if (s->own_stream && s->stream) (void) hipStreamDestroy (s->stream);
      s->shared->clones--;
      delete s;
      return;
   }
   if (s->trans_of) trans_detach (s);
   if (s->trans) trans_release (s);      // before the stream it shares goes
   valgrad_release (s);
   valprod_release (s);
   residual_release (s);
   for (nkp_solver *c : s->batch_members) solver_free (c);
   s->batch_members.clear ();
   for (double *p : { s->bvin, s->bz, s->bw })
      if (p) (void) hipFree (p);
   void *ptrs[] = { s->A.rowptr, s->A.colind, s->A.val, s->A.rowblk, s->A.codes, s->A.dict, s->A.dict_ptr, s->A.dg_ptr, s->A.dg_key, s->A.dg_voff, s->A.dg_vald, s->A.dg_tile, s->A.dg_gptr, s->A.dg_grp, s->B.blk_start, s->B.fac, s->B.grp_b0, s->B.grp_nb, s->B.grp_maxlen, s->B.grp_base, s->B.grp_row0, s->B.col_slot, s->B.fac_t, s->B.gs_rb_ptr, s->B.gs_rb, s->V, s->vcur, s->Z, s->w, s->r,
                    s->x, s->b, s->t1, s->t2, s->p1, s->p2, s->partial, s->dscal, s->dint, s->rscale, s->rinv, s->eqtmp };
   for (void *p : ptrs)
      if (p) (void) hipFree (p);
   delete s->B.grp_cols;
   ml_free (s->ml);
   if (s->rf) { rf_free (*s->rf); delete s->rf; }
   if (s->dplan) { rf_dist_free (*s->dplan); delete s->dplan; }
   s->dist.each_exchange ([] (RowExchange &X, bool) { exchange_release (X); });
   for (void *p : { (void *) s->dist.xe, (void *) s->dist.sel_idx, (void *) s->dist.rext, (void *) s->dist.zext, (void *) s->dist.bxe, (void *) s->dist.gmsg })
      if (p) (void) hipFree (p);
   if (s->dist.ghpin) (void) hipHostFree (s->dist.ghpin);
   if (s->dist.ev_packed) (void) hipEventDestroy (s->dist.ev_packed);
   if (s->dist.ev_halo) (void) hipEventDestroy (s->dist.ev_halo);
   if (s->dist.comm_stream) (void) hipStreamDestroy (s->dist.comm_stream);
   if (s->hpin) (void) hipHostFree (s->hpin);
   if (s->own_stream && s->stream) (void) hipStreamDestroy (s->stream);
   delete s;
}

extern "C" void nkp_destroy (nkp_solver *s) { solver_free (s); }

void msg (const nkp_solver *s, int lvl, const char *fmt, ...)
{
   if (s->opt.verbose < lvl) return;
   va_list ap;
   va_start (ap, fmt);
   printf ("(%d) ", s->opt.rank);
   vprintf (fmt, ap);
   va_end (ap);
   fflush (stdout);
}

extern "C" int nkp_set_stream (nkp_solver *s, void *hip_stream)
{
   if (!s) return fail (NKP_EINVAL, "nkp_set_stream: NULL solver");
   if (s->trans_of) return fail (NKP_EINVAL, "nkp_set_stream: a transposed solver runs on the stream of the solver it was transposed from; set that one's stream");
   if (s->own_stream && s->stream) { (void) hipStreamSynchronize (s->stream); (void) hipStreamDestroy (s->stream); }
   // NULL is a stream too: the device's default stream (what torch.cuda.current_stream() is unless the
   // caller switched streams), so work enqueued here stays ordered with the caller's own kernels
   s->stream = (hipStream_t) hip_stream;
   s->own_stream = false;
   for (nkp_solver *c : s->batch_members) c->stream = s->stream;      // the members of a batch share the solver's stream
   trans_set_stream (s);                                               // ... and so does the transposed solver
   return NKP_OK;
}

extern "C" int64_t nkp_get_int (nkp_solver *s, const char *key)
{
   if (!s || !key) return -1;
   if (!strcmp (key, "n")) return s->n;
   if (!strcmp (key, "nnz")) return s->A.nnz;
   if (!strcmp (key, "nblk")) return s->B.nblk;
   if (!strcmp (key, "band")) return s->B.P;
   if (!strcmp (key, "band_dropped")) return s->B.dropped;
   if (!strcmp (key, "col_stream")) return s->B.stream ? 1 : 0;
   if (!strcmp (key, "col_ldsres")) return s->B.ldsres;
   if (!strcmp (key, "col_gw")) return s->B.gw;
   if (!strcmp (key, "col_max_len")) return s->B.max_len;
   if (!strcmp (key, "col_lds_bytes")) return (int64_t) s->B.lds_doubles * (int64_t) sizeof (double);
   if (!strcmp (key, "levels")) return s->opt.precond == NKP_PRECOND_MULTILEVEL ? (int64_t) s->ml.lev.size () : 1;
   if (!strcmp (key, "ml_rows")) { int64_t t = 0; for (auto &v : s->ml.lev) t += v.n; return t; }
   if (!strcmp (key, "ml_nnz")) { int64_t t = 0; for (auto &v : s->ml.lev) t += v.L.nnz; return t; }
   if (!strcmp (key, "rowblocks")) return s->A.nrowblk;
   if (!strcmp (key, "spmv_bytes")) return 12 * s->A.nnz + 4 * (s->n + 1) + 16 * s->n;
   if (!strcmp (key, "spmv_diag")) return s->A.dg_vald ? 1 : 0;
   // compulsory bytes of one product on the diagonals, counted as ml_bytes counts a level's: values, tiles, groups, x and y
   if (!strcmp (key, "spmv_diag_bytes"))
      return s->A.dg_vald ? 8 * s->A.dg_nval + (int64_t) s->A.dg_ntile * (int64_t) sizeof (DgTile) + (int64_t) s->A.dg_ngrp * (int64_t) sizeof (DgGroup) + 16 * s->n : 0;
   if (!strcmp (key, "precond_bytes")) return s->opt.precond == NKP_PRECOND_NONE ? 16 * s->n : (int64_t) (2 * s->B.P + 1) * 8 * s->n + 16 * s->n;
   if (!strcmp (key, "device_bytes")) return (int64_t) s->device_bytes;
   if (!strcmp (key, "precond_steps")) return s->precond_steps;
   if (!strcmp (key, "max_iters")) return s->opt.max_iters;
   if (!strcmp (key, "equil")) return s->equil ? 1 : 0;
   if (!strcmp (key, "dist_overlap")) return s->dist.overlap ? 1 : 0;
   if (!strcmp (key, "dist_ras")) return s->dist.ras ? 1 : 0;
   if (!strcmp (key, "dist_ras_rows")) return s->dist.n_sel;
   if (!strcmp (key, "dist_ras_rings")) return s->dist.ras ? s->dist.ras_rings : 0;
   if (!strcmp (key, "dist_halo_rows")) return s->dist.n_halo;
   if (!strcmp (key, "dist_smooth_exchange")) return s->dist.smooth ? 1 : 0;
   if (!strcmp (key, "dist_smooth_rows")) return s->dist.smooth ? s->dist.n_sel : 0;
   // rows received per preconditioner application: the SpMV halo with one ring, the overlap rows alone with more
   if (!strcmp (key, "dist_ras_recv_rows")) return !s->dist.ras ? 0 : s->dist.ras_sep ? s->dist.n_sel : s->dist.n_halo;
   if (!strcmp (key, "dist_interior_rowblocks")) return s->dist.seg_rb[2] - s->dist.seg_rb[1];
   if (!strcmp (key, "smoother_spmv_bytes")) return s->opt.precond == NKP_PRECOND_MULTILEVEL ? ml_bytes (s->ml, 0) : 0;
   if (!strcmp (key, "column_solve_bytes")) return s->opt.precond == NKP_PRECOND_MULTILEVEL ? ml_bytes (s->ml, 1) : 0;
   if (!strcmp (key, "cycle_bytes")) return s->opt.precond == NKP_PRECOND_MULTILEVEL ? ml_bytes (s->ml, 2) : 0;
   if (!strcmp (key, "ml_levels_on_device")) return s->ml.levels_on_device;
   if (!strcmp (key, "ml_inverse_pivoted")) return s->ml.inverse_pivoted;
   if (!strcmp (key, "ml_setup_us")) return (int64_t) (s->ml.setup_seconds * 1.0e6);
   if (!strcmp (key, "create_us")) return (int64_t) (s->create_seconds * 1.0e6);
   if (!strcmp (key, "refactor_count")) return s->refactor_count;
   if (!strcmp (key, "refactor_rebuilt")) return s->refactor_rebuilt;
   if (!strcmp (key, "refactor_us")) return (int64_t) (s->refactor_seconds * 1.0e6);
   if (!strcmp (key, "refactor_halo_values")) return s->refactor_halo_values;
   if (!strcmp (key, "is_transpose")) return s->trans_of ? 1 : 0;
   if (!strcmp (key, "trans_device_bytes")) return trans_device_bytes (s);
   if (!strcmp (key, "trans_us")) return (int64_t) (s->trans_seconds * 1.0e6);
   if (!strcmp (key, "trans_kernel_us")) return (int64_t) (s->trans_kernel_seconds * 1.0e6);
   if (!strcmp (key, "trans_sent_entries")) return s->trans_sent;
   if (!strcmp (key, "trans_recv_entries")) return s->trans_received;
   if (!strcmp (key, "dist_alltoallv_calls")) return s->shared->alltoallv_calls.load ();
   if (!strcmp (key, "dist_allreduce_calls")) return s->shared->allreduce_calls.load ();
   if (!strcmp (key, "value_gradient_calls")) return s->vg.calls;
   if (!strcmp (key, "value_gradient_us")) return (int64_t) (s->vg.seconds * 1.0e6);
   if (!strcmp (key, "values_product_calls")) return s->vp.calls;
   if (!strcmp (key, "values_product_us")) return (int64_t) (s->vp.seconds * 1.0e6);
   if (!strcmp (key, "tangent_calls")) return s->vp.tangent_calls;
   if (!strcmp (key, "residual_batch_calls")) return s->rb.calls;
   if (!strcmp (key, "residual_batch_us")) return (int64_t) (s->rb.seconds * 1.0e6);
   if (!strcmp (key, "values_product_trans_calls")) return s->vt.calls;
   if (!strcmp (key, "values_product_trans_us")) return (int64_t) (s->vt.seconds * 1.0e6);
   if (!strcmp (key, "trans_index_bytes")) return (int64_t) s->vt.bytes;
   if (!strcmp (key, "trans_index_us")) return (int64_t) (s->vt.build_seconds * 1.0e6);
   if (!strcmp (key, "trans_index_sent_entries")) return s->vt.n_ship;
   if (!strcmp (key, "trans_index_recv_entries")) return s->vt.n_recv;
   if (!strcmp (key, "batch_steps")) return s->batch_steps;
   if (!strcmp (key, "batch_width")) return s->batch_width;
   if (!strcmp (key, "batch_member_bytes")) {      // the further sets of work vectors a batched group keeps (not part of device_bytes)
      size_t sum = 0;
      for (const nkp_solver *c : s->batch_members) sum += c->device_bytes;
      return (int64_t) sum;
   }
   return -1;
}

extern "C" int nkp_set_device (int device)
{
   HIPCHK (hipSetDevice (device));
   return NKP_OK;
}
