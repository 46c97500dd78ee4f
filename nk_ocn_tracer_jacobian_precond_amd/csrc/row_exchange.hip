// What a row-distributed solver does with an exchange of rows (row_exchange.h): its device memory, the
// collective itself -- every alltoallv of a solve is the one in exchange_rows -- and the halo fetch in front of a product with A.
#include "solver_impl.h"

bool exchange_install (nkp_solver *s, RowExchange &X, const int32_t *rows, const std::vector<int> &give, const std::vector<int> &need,
                       bool unpacks, int64_t cap_send, int64_t cap_recv, int64_t wide_recv)
{
   X.send_counts = give; X.recv_counts = need;
   for (int c : give) X.nsend += c;
   for (int c : need) X.nrecv += c;
   X.wide_send = cap_send; X.wide_recv = wide_recv;
   bool ok = dev_alloc (s, &X.send_idx, (size_t) X.nsend) == NKP_OK;
   if (ok && unpacks) ok = dev_alloc (s, &X.recv_idx, (size_t) X.nrecv) == NKP_OK;
   if (ok && cap_send >= 0) ok = dev_alloc (s, &X.send, (size_t) cap_send) == NKP_OK;
   if (ok && cap_recv >= 0) ok = dev_alloc (s, &X.recv, (size_t) cap_recv) == NKP_OK;
   if (ok && rows && X.nsend) ok = hipMemcpy (X.send_idx, rows, (size_t) X.nsend * sizeof (int), hipMemcpyHostToDevice) == hipSuccess;
   return ok;
}

void exchange_release (RowExchange &X)
{
   for (void *p : { (void *) X.send_idx, (void *) X.recv_idx, (void *) X.send, (void *) X.recv, (void *) X.bsend, (void *) X.brecv })
      if (p) (void) hipFree (p);
}

int halo_fetch (nkp_solver *s, int K, const double *x, const double *const *xp, hipStream_t comm, bool sticky)
{
   auto &D = s->dist;
   RowExchange &X = D.x_halo;
   hipStream_t st = s->stream;
   if (K == 1 && xp) x = xp[0];
   if (K == 1) launch_copy (x, D.xe, s->n, st);
   else if (xp) launch_interleave (K, xp, D.bxe, s->n, st);
   if (X.nsend && K == 1) launch_gather (X.send_idx, x, X.send_for (K), X.nsend, st);
   else if (X.nsend && xp) launch_gather_interleave (K, X.send_idx, xp, X.send_for (K), X.nsend, st);
   else if (X.nsend) launch_gather_batch (K, X.send_idx, x, X.send_for (K), X.nsend, st);
   if (comm != st) {
      (void) hipEventRecord (D.ev_packed, st);
      (void) hipStreamWaitEvent (comm, D.ev_packed, 0);
   }
   const int rc = exchange_rows (s, X, K, X.send_for (K), halo_rows_of (s, K), comm, sticky);
   if (comm != st) (void) hipEventRecord (D.ev_halo, comm);
   return rc;
}
