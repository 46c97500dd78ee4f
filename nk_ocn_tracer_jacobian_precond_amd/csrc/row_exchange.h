// One exchange of rows between the ranks of a row-distributed solver (what is done with it: row_exchange.hip).  No HIP here.
#pragma once
#include <stdint.h>

#include <vector>

// which own rows go out (by destination rank), how many rows every rank sends and receives, and the buffers they pass through --
// one row wide and, for K interleaved systems, K rows wide.  A copy shares the device memory with the exchange it was copied
// from, which frees it (a batch member is a copy of its parent); the counts and their cache are the copy's own.  An exchange
// may have no buffers and pass through another's (the two colours of the fine-level exchange never run at once).
struct RowExchange {
   int64_t nsend = 0, nrecv = 0;
   std::vector<int> send_counts, recv_counts;     // rows per rank (the plan's)
   int *send_idx = nullptr;                       // device: the rows sent, grouped by destination
   int *recv_idx = nullptr;                       // device: where arriving rows go, where the exchange unpacks (fine-level exchange)
   double *send = nullptr, *recv = nullptr;       // one row wide; recv stays NULL where rows land in a vector of the caller's
   double *bsend = nullptr, *brecv = nullptr;     // K wide (batch_prepare_exchange), for K <= the solver's dist.bK
   int64_t wide_send = -1, wide_recv = -1;        // rows bsend / brecv are to hold (exchange_install), -1: no such buffer
   double *send_for (int K) const { return K == 1 ? send : bsend; }
   double *recv_for (int K) const { return K == 1 ? recv : brecv; }
   // K = 1: the plan's counts; K = 2, 4, 8: times K, recomputed only when K changes
   const int *send_counts_for (int K) { return K == 1 ? send_counts.data () : (scale (K), send_k.data ()); }
   const int *recv_counts_for (int K) { return K == 1 ? recv_counts.data () : (scale (K), recv_k.data ()); }
   void drop_wide () { bsend = brecv = nullptr; scaled_K = 0; }      // a copy that works one row wide: the K-wide buffers stay with the original

private:
   int scaled_K = 0;
   std::vector<int> send_k, recv_k;
   void scale (int K)
   {
      if (K == scaled_K) return;
      send_k = send_counts;
      recv_k = recv_counts;
      for (int &v : send_k) v *= K;
      for (int &v : recv_k) v *= K;
      scaled_K = K;
   }
};
