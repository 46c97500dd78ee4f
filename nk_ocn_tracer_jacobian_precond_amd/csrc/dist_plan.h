// Host-side plan of the row-distributed flavour (dist_plan.cpp): plain C++, no HIP.  Private to the library: nothing here is
// part of the C ABI, so everything is hidden from the dynamic symbol table.
#pragma once
#include "../../include/nkp.h"
#include "tuning.h"

#include <stdint.h>

#include <string>
#include <vector>

// ---- the plan ---------------------------------------------------------------------------------------------------------------
struct DistPlan {
   std::vector<int32_t> colind_ext, halo_rows, send_rows, need, give;     // SpMV: renumbered columns, halo rows in, own rows out
   int64_t n_halo = 0, nsend = 0;
   std::vector<int32_t> e_rowptr, e_colind, e_blk, e_ci, e_cj, e_ct, sel_hpos;   // hierarchy on [own rows | overlap rows]
   std::vector<double> e_val;
   int64_t n_sel = 0;
   bool ras = false;
   // what nkp_refactor_dist needs to redo the value part: where every entry of e_* comes from (own local entry e, or
   // -1 - position in the received overlap values), the own entries shipped (in val_s order) and the entry counts per rank
   std::vector<int32_t> e_org, ship_e;
   std::vector<int> ent_give, ent_need;
   // the depth the ranks agreed on (0: no overlap); with two or more rings the overlap rows are not all in the SpMV halo and
   // the residual of the cycle has an exchange of its own: own local rows sent (by destination, ascending), rows per rank
   int rings = 0;
   std::vector<int32_t> ras_send_rows;
   std::vector<int> ras_need, ras_give;
   // fine-level exchange (tuning dist_smooth_exchange, the smallest value any rank asked for; 0 without overlap): per colour
   // c = (i + j) % 2 of the water columns' grid positions, the own local rows other ranks hold as overlap rows (all rings; by
   // destination, ascending), the rows per rank both ways, and this rank's overlap rows of that colour as rows of the hierarchy's
   // matrix (>= m_loc) in its order, which is the order they arrive in
   int smooth = 0;
   std::vector<int32_t> smooth_send_rows[2], smooth_recv_rows[2];
   std::vector<int> smooth_give[2], smooth_need[2];
};

// Everything nkp_create_dist decides before a byte goes to the device.  Collective over the ranks through the host callbacks
// of `comm`; starts[nranks + 1] are the first rows of all ranks.
NKP_PRIVATE int dist_plan (DistPlan &D, const nkp_comm_ops *comm, const nkp_options &o, const std::vector<int64_t> &starts, int64_t fst_row,
                           int64_t m_loc, int64_t nnz_loc, const int32_t *rowptr_loc, const int32_t *colind_glob, const double *val,
                           const int32_t *blk_start_loc, int64_t nblk_loc, int coupled_tracer_cnt);

// All ranks learn whether any rank failed a check that only one rank can fail, and leave together: a rank that returned alone
// would leave its peers blocked in the next exchange, for good with a transport that has no deadline (RCCL).  A rank that failed
// keeps its code and message; the others get NKP_ECOMM "<who>: rank <p> failed its checks (<where>); see its message".  A
// failed allgather is NKP_ECOMM on every rank.
NKP_PRIVATE int dist_agree_checks (const nkp_comm_ops *comm, int local_rc, const char *who, const char *where);
