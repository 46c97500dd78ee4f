// RowExchange (csrc/row_exchange.h) alone, built with the address and undefined-behaviour sanitizers: the counts an exchange hands
// to the transport at every interleave width, and what a copy shares with its original.  No GPU: the "device" pointers are
// addresses of host arrays and are only compared.  Prints "ok" and returns 0, or names the first check that failed.
#include "row_exchange.h"

#include <stdio.h>

static int failures = 0;

#define CHECK(cond)                                                     \
   do {                                                                 \
      if (!(cond)) { printf ("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
   } while (0)

static bool is_scaled (const int *got, const std::vector<int> &plan, int K)
{
   for (size_t p = 0; p < plan.size (); p++)
      if (got[p] != plan[p] * K) return false;
   return true;
}

static void check_widths (RowExchange &X, const std::vector<int> &give, const std::vector<int> &need)
{
   // one row wide: the plan's own vectors, not a copy of them
   CHECK (X.send_counts_for (1) == X.send_counts.data () && X.recv_counts_for (1) == X.recv_counts.data ());
   for (int K : { 2, 4, 8 }) CHECK (is_scaled (X.send_counts_for (K), give, K) && is_scaled (X.recv_counts_for (K), need, K));
   // widening and narrowing on a live exchange; the two sides may be asked in either order
   for (int K : { 4, 2, 8, 1, 4 }) {
      CHECK (is_scaled (X.recv_counts_for (K), need, K));
      CHECK (is_scaled (X.send_counts_for (K), give, K));
      CHECK (X.send_counts == give && X.recv_counts == need);      // the plan's counts are never touched
   }
}

int main ()
{
   const std::vector<int> give = { 0, 3, 0, 7, 1 }, need = { 0, 0, 5, 2, 0 };      // (with zeros: ranks that exchange nothing)
   RowExchange X;
   X.send_counts = give;
   X.recv_counts = need;
   check_widths (X, give, need);

   // one rank: no counts at all
   RowExchange E;
   check_widths (E, {}, {});
   for (int K : { 1, 2, 8 }) (void) E.send_counts_for (K), (void) E.recv_counts_for (K);

   // a copy shares the pointers; drop_wide () clears the copy's K-wide ones only, and the copy scales on its own
   int idx[2];
   double one[2], wide[16];
   X.send_idx = idx; X.recv_idx = idx + 1;
   X.send = one; X.recv = one + 1;
   X.bsend = wide; X.brecv = wide + 8;
   const int *x_send8 = X.send_counts_for (8);
   RowExchange C = X;
   C.drop_wide ();
   CHECK (C.send_idx == idx && C.recv_idx == idx + 1 && C.send == one && C.recv == one + 1 && C.bsend == nullptr && C.brecv == nullptr);
   CHECK (C.send_for (1) == one && C.recv_for (1) == one + 1 && C.send_for (4) == nullptr);
   CHECK (X.send_idx == idx && X.recv_idx == idx + 1 && X.send == one && X.recv == one + 1 && X.bsend == wide && X.brecv == wide + 8);
   CHECK (X.send_for (8) == wide && X.recv_for (2) == wide + 8);
   const int *c_send2 = C.send_counts_for (2);
   CHECK (c_send2 != x_send8 && is_scaled (c_send2, give, 2) && is_scaled (C.recv_counts_for (2), need, 2));
   CHECK (X.send_counts_for (8) == x_send8 && is_scaled (x_send8, give, 8) && is_scaled (X.recv_counts_for (8), need, 8));      // the original's cache: untouched
   check_widths (C, give, need);
   CHECK (is_scaled (X.send_counts_for (8), give, 8));

   if (!failures) printf ("ok\n");
   return failures ? 1 : 0;
}
