// What nkp_transpose_dist (transpose_dist.hip) and the transposed index of nkp_values_product_trans_dist (valprod_trans_dist.hip)
// share: the local transpose of a rank's [own | halo] rectangle, the exchange of the entry counts of the halo rows, the placement
// plan of the assembled row block of A^T and the two kernels that place by it.  Private to the library.
#pragma once
#include "solver_impl.h"
#include "transpose.h"

// what one build holds between its steps; everything on the device is freed when it goes out of scope
struct NKP_PRIVATE TransDistBuild {
   int P = 1, me = 0;
   int64_t m_loc = 0, n_halo = 0, nnz = 0, n_own = 0, n_ship = 0, n_recv = 0, nnzF = 0, nseg = 0;
   mls::DBuf<int> rowptrT, colindT, src, colF, origin, ship;
   mls::DBuf<double> valT, valF, recv_val;
   std::vector<int32_t> h_rpT, cnt_send, cnt_recv, ship_glob, recv_col, rowptrF, own_dst, seg_ptr, seg_dst, h_colF;
   std::vector<int> ent_send, ent_recv;
   std::vector<double> h_valF;
   double kernel_seconds = 0.0;
   explicit TransDistBuild (const nkp_solver *s)
      : P (s->dist.ops.nranks), me (s->dist.ops.rank), m_loc (s->n), n_halo (s->dist.n_halo), nnz (s->A.nnz), nseg (s->dist.x_halo.nsend) {}
};

// Every step is rank-local unless it says otherwise, names `who` in its messages and returns an NKP_ code; the agreement after a
// step carries a failure to the peers.
// step 1: the rectangular transpose on the device (rowptrT, colindT, valT, src; rows >= m_loc are the send stream, grouped by owner),
// its row offsets on the host, n_own, n_ship, the entry count of every halo row (cnt_send) and of every owner (ent_send)
NKP_PRIVATE int td_local_transpose (nkp_solver *s, TransDistBuild &B, const char *who);
// step 2, COLLECTIVE (one alltoallv_i32_host; the ranks agreed before it that step 1 succeeded everywhere): the entry counts of the
// halo rows to their owners, cnt_recv[k] for the k-th row a peer holds as halo
NKP_PRIVATE int td_exchange_counts (nkp_solver *s, TransDistBuild &B, const char *who);
// step 3: n_recv, ent_recv, the row offsets rowptrF of the assembled block and where every contribution starts -- own_dst per own
// row, seg_ptr / seg_dst per received segment; the contributions of a row follow each other in rank order
NKP_PRIVATE int td_plan_placement (nkp_solver *s, TransDistBuild &B, const char *who);
// step 4: colF and origin (and valF with values) of the assembled block by the plan, enqueued on the solver's stream.  An own entry
// gets the column own_add + its local source row, its value and origin = its position in the source's values; received entry i
// gets the column recv_col[i] (B.recv_col, uploaded here) with values, recv_add + i without, the value recv_val[i] and origin = -1 - i.
// Synchronises the stream
NKP_PRIVATE int td_place_entries (nkp_solver *s, TransDistBuild &B, bool values, int own_add, int recv_add, const char *who);
