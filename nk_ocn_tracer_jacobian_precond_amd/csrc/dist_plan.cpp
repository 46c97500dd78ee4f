// Host-side plan of the row-distributed flavour: everything nkp_create_dist decides before a byte goes to the device -- the halo
// of the SpMV, and, with grid positions, the overlap of the hierarchy (halo columns completed to whole water columns, which of
// them are lateral neighbours, their matrix rows fetched from the owners, ring by ring).  Collective over the ranks through the
// host callbacks of nkp_comm_ops; plain C++ without a HIP call, so the N > 1 logic is built and tested without a GPU
// (nkp_dist_overlap_plan_host, tests/test_dist_gloo.py, tests/test_dist_rings.py).  Also the two host-only helpers of the
// cell-major partition.
#include "dist_plan.h"

#include <string.h>

#include <algorithm>
#include <thread>

extern "C" int nkp_dist_plan_host (int64_t m_loc, int64_t nnz_loc, const int32_t *rowptr_loc, const int32_t *colind_glob,
                                   int rank, int nranks, const int64_t *starts, int32_t *colind_ext, int32_t *halo_rows,
                                   int64_t *n_halo, int32_t *need_counts)
{
   if (!rowptr_loc || !starts || !colind_ext || !halo_rows || !n_halo || !need_counts || rank < 0 || rank >= nranks)
      return fail (NKP_EINVAL, "nkp_dist_plan_host: bad argument");
   if (nnz_loc > 0 && !colind_glob) return fail (NKP_EINVAL, "nkp_dist_plan_host: bad argument");
   const int64_t fst = starts[rank], n_global = starts[nranks];
   if (starts[rank + 1] - fst != m_loc || rowptr_loc[0] != 0 || rowptr_loc[m_loc] != nnz_loc)
      return fail (NKP_EINVAL, "nkp_dist_plan_host: starts[] / rowptr_loc inconsistent with m_loc, nnz_loc");
   // sorted unique off-rank columns
   std::vector<int32_t> off;
   for (int64_t e = 0; e < nnz_loc; e++) {
      const int64_t c = colind_glob[e];
      if (c < 0 || c >= n_global) return fail (NKP_EINVAL, "nkp_dist_plan_host: column index %lld out of range", (long long) c);
      if (c < fst || c >= fst + m_loc) off.push_back ((int32_t) c);
   }
   std::sort (off.begin (), off.end ());
   off.erase (std::unique (off.begin (), off.end ()), off.end ());
   *n_halo = (int64_t) off.size ();
   for (int p = 0; p < nranks; p++) need_counts[p] = 0;
   {
      int p = 0;
      for (size_t q = 0; q < off.size (); q++) {
         while (off[q] >= starts[p + 1]) p++;           // sorted rows, ascending owners
         need_counts[p]++;
         halo_rows[q] = off[q];
      }
   }
   for (int64_t e = 0; e < nnz_loc; e++) {
      const int64_t c = colind_glob[e];
      if (c >= fst && c < fst + m_loc) colind_ext[e] = (int32_t) (c - fst);
      else colind_ext[e] = (int32_t) (m_loc + (std::lower_bound (off.begin (), off.end (), (int32_t) c) - off.begin ()));
   }
   return NKP_OK;
}

int dist_agree_checks (const nkp_comm_ops *comm, int local_rc, const char *who, const char *where)
{
   std::vector<int64_t> all ((size_t) comm->nranks + 1, 0);
   const std::string mine = local_rc ? last_error_message () : std::string ();
   if (comm->allgather_i64_host (comm->ctx, local_rc ? 1 : 0, all.data ())) return fail (NKP_ECOMM, "%s: allgather failed (%s)", who, where);
   if (local_rc) { restore_error_message (mine); return local_rc; }
   for (int p = 0; p < comm->nranks; p++)
      if (all[(size_t) p]) return fail (NKP_ECOMM, "%s: rank %d failed its checks (%s); see its message", who, p, where);
   return NKP_OK;
}

namespace {

// One call of dist_plan: its arguments, what the steps hand to each other, and one method per step.  Every exchange buffer is
// one element longer than its message, so that .data () of an empty message is a valid pointer.
struct Planner {
   DistPlan &D;
   const nkp_comm_ops *comm;
   const nkp_options &o;
   const std::vector<int64_t> &starts;
   const int64_t fst_row, m_loc, nnz_loc;
   const int32_t *rowptr_loc, *colind_glob;
   const double *val;
   const int32_t *blk_start_loc;
   const int64_t nblk_loc;
   const int coupled_tracer_cnt, P = comm->nranks, rank = comm->rank;
   const std::vector<int32_t> ones = std::vector<int32_t> ((size_t) P, 1);

   int64_t rings = 0;                                      // the depth the ranks agreed on (0: no overlap)
   std::vector<int32_t> col_of;                            // own local row -> own water column
   std::vector<int64_t> own_pos;                           // (j, i) of the own columns, sorted
   // One ring's answer to "complete these rows to whole water columns".  Owner side: the own columns and their rows shipped,
   // by destination.  Requester side: the global ids of the completed rows, column after column, and (length, i, j) of every
   // column, by owner.
   struct Completed {
      std::vector<int32_t> out_rows, out_cols, rows_r, meta_r;
      std::vector<int> give_rows, give_cols, need_rows, need_cols;          // per rank
      int64_t n_rows = 0, n_cols = 0;
      explicit Completed (int P) : give_rows (P, 0), give_cols (P, 0), need_rows (P, 0), need_cols (P, 0) {}
   };
   // The overlap so far.  What arrives is kept per row and ordered once all rings are in.
   struct OvCol { int32_t g0; int len, ci, cj, ring; int64_t row0; };
   std::vector<OvCol> ocols;
   std::vector<int32_t> arr_gid, arr_col;                  // per arrived row: global id; per entry: global column
   std::vector<int64_t> arr_ptr = std::vector<int64_t> (1, 0);
   std::vector<double> arr_val;
   std::vector<int> ring_first = std::vector<int> (1, 0);  // first arrived row of every ring
   std::vector<int32_t> ov_sorted;                         // global rows of the rings before the current one, ascending
   std::vector<std::vector<int32_t>> shipped = std::vector<std::vector<int32_t>> ((size_t) P);   // owner: own local rows shipped to each rank over all rings
   int64_t n_sel_all = 0;                                  // rows received over all rings
   int64_t smooth = 0;                                     // the fine-level exchange the ranks agreed on (0 / 1)
   std::vector<int> ov_need;                               // overlap rows per owner (hierarchy order = ascending owners)

   int agree (int local_rc, const char *where) { return dist_agree_checks (comm, local_rc, "nkp_create_dist", where); }
   int exchange (const int32_t *sendp, const int *scnt, int32_t *recvp, const int *rcnt, const char *what) {
      return comm->alltoallv_i32_host (comm->ctx, sendp, scnt, recvp, rcnt) ? fail (NKP_ECOMM, "nkp_create_dist: %s exchange failed", what) : NKP_OK;
   }
   bool owned (int64_t g) const { return g >= fst_row && g < fst_row + m_loc; }

   // ---- step 1: the SpMV halo and the rows every peer reads from this rank
   int spmv_halo ()
   {
      D.colind_ext.assign ((size_t) nnz_loc + 1, 0);
      D.halo_rows.assign ((size_t) nnz_loc + 1, 0);
      D.need.assign (P, 0);
      D.give.assign (P, 0);
      int rc = (starts[(size_t) rank + 1] - starts[(size_t) rank] != m_loc)
                  ? fail (NKP_EINVAL, "nkp_create_dist: m_loc = %lld does not match the next rank's fst_row", (long long) m_loc)
                  : nkp_dist_plan_host (m_loc, nnz_loc, rowptr_loc, colind_glob, rank, P, starts.data (), D.colind_ext.data (), D.halo_rows.data (), &D.n_halo, D.need.data ());
      if ((rc = agree (rc, "local rows and halo plan"))) return rc;
      // tell every owner how many and which of its rows this rank reads
      if ((rc = exchange (D.need.data (), ones.data (), D.give.data (), ones.data (), "count"))) return rc;
      for (int p = 0; p < P; p++) D.nsend += D.give[p];
      D.send_rows.assign ((size_t) D.nsend + 1, 0);
      if ((rc = exchange (D.halo_rows.data (), D.need.data (), D.send_rows.data (), D.give.data (), "index"))) return rc;
      for (int64_t q = 0; q < D.nsend; q++) {
         D.send_rows[q] -= (int32_t) fst_row;
         if (D.send_rows[q] < 0 || D.send_rows[q] >= m_loc) rc = fail (NKP_ECOMM, "nkp_create_dist: a peer asked for a row this rank does not own");
      }
      return agree (rc, "requested rows");
   }

   // ---- step 2: the depth this rank asks for rides on the message that decides the overlap (0 = none); the ranks take the
   // smallest.  -1 = a knob out of range: every rank refuses it together.  The fine-level exchange a rank asks for (tuning
   // dist_smooth_exchange) is the lowest bit of the same message, and again the smallest holds
   int agree_on_depth ()
   {
      const bool geo = o.col_i && o.col_j && blk_start_loc && nblk_loc > 0;
      int64_t want_ras = (o.precond == NKP_PRECOND_MULTILEVEL && geo) ? 1 : 0;
      rings = 1;
      nkp_tuning tune;
      bool range_error = false;
      if (resolve_tuning (&o, &tune, &range_error) == NKP_OK) {      // a struct of the wrong size is reported by the create call itself
         if (!tune.dist_ras) want_ras = 0;
         rings = tune.dist_ras_rings > 0 ? tune.dist_ras_rings : 1;
         smooth = tune.dist_smooth_exchange == 1 ? want_ras : 0;
      }
      const std::string mine = range_error ? last_error_message () : std::string ();
      std::vector<int64_t> all (P + 1, 0);
      if (comm->allgather_i64_host (comm->ctx, range_error ? -1 : 2 * want_ras * rings + smooth, all.data ())) return fail (NKP_ECOMM, "nkp_create_dist: allgather failed");
      if (range_error) { restore_error_message (mine); return NKP_EINVAL; }
      for (int p = 0; p < P; p++)
         if (all[p] < 0) return fail (NKP_ECOMM, "nkp_create_dist: rank %d failed its checks (tuning); see its message", p);
      for (int p = 0; p < P; p++) { rings = std::min (rings, all[p] >> 1); smooth = std::min (smooth, all[p] & 1); }
      return NKP_OK;
   }

   // ---- step 3, rings >= 2: the rows of other ranks that the last ring couples to, in no ring yet, go to their owners as
   // requests.  (Ring 1 has no such round: its requests are the SpMV halo exchange of step 1.)  wanted: the global rows asked
   // for (ascending, padded); req / req_give: the own local rows the peers ask this rank for, by requester
   int request_ring (int ring, std::vector<int32_t> &wanted, std::vector<int32_t> &req, std::vector<int> &req_give)
   {
      ov_sorted.assign (arr_gid.begin (), arr_gid.end ());
      std::sort (ov_sorted.begin (), ov_sorted.end ());
      for (int a = ring_first[ring - 2]; a < ring_first[ring - 1]; a++)
         for (int64_t e = arr_ptr[a]; e < arr_ptr[a + 1]; e++) {
            const int32_t g = arr_col[(size_t) e];
            if (!owned (g) && !std::binary_search (ov_sorted.begin (), ov_sorted.end (), g)) wanted.push_back (g);
         }
      std::sort (wanted.begin (), wanted.end ());
      wanted.erase (std::unique (wanted.begin (), wanted.end ()), wanted.end ());
      std::vector<int> req_need (P, 0);
      req_give.assign (P, 0);
      for (int32_t g : wanted) req_need[(size_t) (std::upper_bound (starts.begin (), starts.begin () + P, (int64_t) g) - starts.begin () - 1)]++;
      int rc;
      if ((rc = exchange (req_need.data (), ones.data (), req_give.data (), ones.data (), "ring request count"))) return rc;
      int64_t n_req = 0;
      for (int p = 0; p < P; p++) n_req += req_give[p];
      req.assign ((size_t) n_req + 1, 0);
      wanted.push_back (0);
      if ((rc = exchange (wanted.data (), req_need.data (), req.data (), req_give.data (), "ring request"))) return rc;
      for (int64_t q = 0; q < n_req; q++) {
         req[(size_t) q] -= (int32_t) fst_row;
         if (req[(size_t) q] < 0 || req[(size_t) q] >= m_loc) rc = fail (NKP_ECOMM, "nkp_create_dist: a peer asked for a ring row this rank does not own");
      }
      return agree (rc, "ring requests");
   }

   // ---- step 3, every ring: the owner completes the requested rows (req: own local rows, req_give[p] of them from rank p) to
   // whole water columns and ships (row ids; length, i, j per column); the requester checks what arrived: ascending rows,
   // lengths adding up, every row it asked for (wanted[0 .. n_wanted), global) present
   int complete_columns (int ring, const int32_t *req, const int *req_give, const int32_t *wanted, int64_t n_wanted, Completed &C)
   {
      const bool first = ring == 1;
      std::vector<int> twos (P, 2), give3 (P), need3 (P);
      std::vector<int32_t> pair_s (2 * (size_t) P), pair_r (2 * (size_t) P);
      size_t q = 0;
      for (int p = 0; p < P; p++) {
         int last = -1;
         for (int k = 0; k < req_give[p]; k++, q++) {
            const int c = col_of[(size_t) req[q]];
            if (c == last) continue;
            last = c;
            C.out_cols.push_back (c);
            C.give_cols[p]++;
            for (int r = blk_start_loc[c]; r < blk_start_loc[c + 1]; r++) { C.out_rows.push_back (r); C.give_rows[p]++; }
         }
         pair_s[2 * (size_t) p] = C.give_rows[p];
         pair_s[2 * (size_t) p + 1] = C.give_cols[p];
      }
      int rc;
      if ((rc = exchange (pair_s.data (), twos.data (), pair_r.data (), twos.data (), first ? "overlap count" : "ring count"))) return rc;
      for (int p = 0; p < P; p++) {
         C.n_rows += C.need_rows[p] = pair_r[2 * (size_t) p];
         C.n_cols += C.need_cols[p] = pair_r[2 * (size_t) p + 1];
         give3[p] = 3 * C.give_cols[p];
         need3[p] = 3 * C.need_cols[p];
      }
      std::vector<int32_t> ids_s (C.out_rows.size () + 1), meta_s (3 * C.out_cols.size () + 1);
      for (size_t k = 0; k < C.out_rows.size (); k++) ids_s[k] = C.out_rows[k] + (int32_t) fst_row;
      C.rows_r.assign ((size_t) C.n_rows + 1, 0);
      if ((rc = exchange (ids_s.data (), C.give_rows.data (), C.rows_r.data (), C.need_rows.data (), first ? "overlap row" : "ring row"))) return rc;
      for (size_t k = 0; k < C.out_cols.size (); k++) {
         const int c = C.out_cols[k];
         meta_s[3 * k] = blk_start_loc[c + 1] - blk_start_loc[c];
         meta_s[3 * k + 1] = o.col_i[c];
         meta_s[3 * k + 2] = o.col_j[c];
      }
      C.meta_r.assign (3 * (size_t) C.n_cols + 1, 0);
      if ((rc = exchange (meta_s.data (), give3.data (), C.meta_r.data (), need3.data (), first ? "overlap column" : "ring column"))) return rc;
      int64_t sum = 0;
      for (int64_t c = 0; c < C.n_cols; c++) sum += C.meta_r[3 * (size_t) c];
      bool good = sum == C.n_rows;
      for (int64_t k = 1; k < C.n_rows && good; k++) good = C.rows_r[(size_t) k] > C.rows_r[(size_t) k - 1];
      for (int64_t k = 0; k < n_wanted && good; k++) good = std::binary_search (C.rows_r.begin (), C.rows_r.begin () + C.n_rows, wanted[k]);
      rc = good ? NKP_OK
           : first ? fail (NKP_ECOMM, "nkp_create_dist: the completed halo is inconsistent (a water column straddles two ranks?)")
                   : fail (NKP_ECOMM, "nkp_create_dist: ring %d is inconsistent (a water column straddles two ranks?)", ring);
      return agree (rc, first ? "completed halo" : "ring columns");
   }

   // ---- step 3, ring 1 only: the SpMV addresses the completed halo from here on
   void install_completed_halo (const Completed &C)
   {
      const auto hbeg = C.rows_r.begin (), hend = C.rows_r.begin () + C.n_rows;
      for (int64_t r = 0; r < m_loc; r++)
         for (int e = rowptr_loc[r]; e < rowptr_loc[r + 1]; e++)
            if (!owned (colind_glob[e])) D.colind_ext[(size_t) e] = (int32_t) (m_loc + (std::lower_bound (hbeg, hend, colind_glob[e]) - hbeg));
      D.n_halo = C.n_rows;
      D.halo_rows = C.rows_r;                                // (with its padding)
      D.need.assign (C.need_rows.begin (), C.need_rows.end ());
      D.give.assign (C.give_rows.begin (), C.give_rows.end ());
      D.nsend = (int64_t) C.out_rows.size ();
      D.send_rows = C.out_rows;
      D.send_rows.push_back (0);
   }

   // ---- step 3, every ring: the requester selects which completed columns join this ring (position not owned here, not in an
   // earlier ring), the owner ships their rows (entries per row, global columns, values as pairs of int32); *n_new: rows received
   int select_and_fetch (int ring, const Completed &C, int64_t *n_new)
   {
      const std::vector<int32_t> &rows_r = C.rows_r, &meta_r = C.meta_r;
      std::vector<int32_t> flag_s ((size_t) C.n_cols + 1, 0), flag_r (C.out_cols.size () + 1, 0);
      std::vector<int> erow_need (P, 0), erow_give (P, 0);
      size_t c = 0, q = 0;
      int64_t hpos = 0;
      for (int p = 0; p < P; p++)
         for (int k = 0; k < C.need_cols[p]; k++, c++) {
            const int64_t key = ((int64_t) meta_r[3 * c + 2] << 32) | (uint32_t) meta_r[3 * c + 1];
            flag_s[c] = std::binary_search (own_pos.begin (), own_pos.end (), key) ? 0 : 1;
            if (flag_s[c] && std::binary_search (ov_sorted.begin (), ov_sorted.end (), rows_r[(size_t) hpos])) flag_s[c] = 0;
            if (flag_s[c]) erow_need[p] += meta_r[3 * c];
            hpos += meta_r[3 * c];
         }
      int rc;
      if ((rc = exchange (flag_s.data (), C.need_cols.data (), flag_r.data (), C.give_cols.data (), "overlap selection"))) return rc;
      std::vector<int32_t> len_s, col_s, val_s;
      std::vector<int> ent_give (P, 0), ent_need (P, 0), ent2_give (P, 0), ent2_need (P, 0);
      c = 0;
      for (int p = 0; p < P; p++)
         for (int k = 0; k < C.give_cols[p]; k++, c++) {
            if (!flag_r[c]) continue;
            const int col = C.out_cols[c];
            for (int r = blk_start_loc[col]; r < blk_start_loc[col + 1]; r++) {
               len_s.push_back (rowptr_loc[r + 1] - rowptr_loc[r]);
               erow_give[p]++;
               shipped[(size_t) p].push_back (r);
               for (int e = rowptr_loc[r]; e < rowptr_loc[r + 1]; e++) {
                  col_s.push_back (colind_glob[e]);
                  int32_t w[2];
                  memcpy (w, &val[e], sizeof (double));
                  val_s.push_back (w[0]);
                  val_s.push_back (w[1]);
               }
               ent_give[p] += rowptr_loc[r + 1] - rowptr_loc[r];
            }
         }
      int64_t n_erow = 0;
      for (int p = 0; p < P; p++) n_erow += erow_need[p];
      std::vector<int32_t> len_r ((size_t) n_erow + 1);
      len_s.push_back (0);
      if ((rc = exchange (len_s.data (), erow_give.data (), len_r.data (), erow_need.data (), "overlap row length"))) return rc;
      int64_t n_eent = 0;
      for (int p = 0; p < P; p++) {
         int64_t t = 0;
         for (int k = 0; k < erow_need[p]; k++, q++) t += len_r[q];
         if (2 * t >= 2147483647LL || 2 * (int64_t) ent_give[p] >= 2147483647LL) { rc = fail (NKP_EINVAL, "nkp_create_dist: overlap rows exceed the int32 exchange counts"); t = 0; ent_give[p] = 0; }
         ent_need[p] = (int) t;
         n_eent += t;
      }
      if ((rc = agree (rc, "overlap sizes"))) return rc;
      for (int p = 0; p < P; p++) { ent2_give[p] = 2 * ent_give[p]; ent2_need[p] = 2 * ent_need[p]; }
      std::vector<int32_t> col_r ((size_t) n_eent + 1), val_r (2 * (size_t) n_eent + 2);
      col_s.push_back (0);
      val_s.push_back (0);
      if ((rc = exchange (col_s.data (), ent_give.data (), col_r.data (), ent_need.data (), "overlap column index"))) return rc;
      if ((rc = exchange (val_s.data (), ent2_give.data (), val_r.data (), ent2_need.data (), "overlap value"))) return rc;
      // requester: keep the selected columns and their rows
      int64_t got = 0;
      size_t rrow = 0;
      c = q = 0;
      hpos = 0;
      for (int p = 0; p < P; p++)
         for (int k = 0; k < C.need_cols[p]; k++, c++) {
            const int len = meta_r[3 * c];
            if (flag_s[c]) {
               ocols.push_back ({ rows_r[(size_t) hpos], len, meta_r[3 * c + 1], meta_r[3 * c + 2], ring, (int64_t) arr_gid.size () });
               for (int t = 0; t < len && rrow < (size_t) n_erow; t++, rrow++) {
                  arr_gid.push_back (rows_r[(size_t) (hpos + t)]);
                  for (int u = 0; u < len_r[rrow]; u++, q++) {
                     double v;
                     memcpy (&v, &val_r[2 * q], sizeof (double));
                     arr_col.push_back (col_r[q]);
                     arr_val.push_back (v);
                  }
                  arr_ptr.push_back ((int64_t) arr_col.size ());
                  got++;
               }
            }
            hpos += len;
         }
      *n_new = got;
      return NKP_OK;
   }

   // ---- step 3: the rings.  Ring 1 = the lateral columns of the completed halo; ring k + 1 = the lateral columns of other
   // ranks, in no earlier ring, that rows of ring k couple to
   int fetch_rings ()
   {
      col_of.assign ((size_t) m_loc + 1, 0);
      for (int64_t c = 0; c < nblk_loc; c++)
         for (int r = blk_start_loc[c]; r < blk_start_loc[c + 1]; r++) col_of[(size_t) r] = (int32_t) c;
      own_pos.resize ((size_t) nblk_loc);
      for (int64_t c = 0; c < nblk_loc; c++) own_pos[(size_t) c] = ((int64_t) o.col_j[c] << 32) | (uint32_t) o.col_i[c];
      std::sort (own_pos.begin (), own_pos.end ());
      int rc;
      int64_t got = 0;
      for (int ring = 1; ring <= rings; ring++) {
         Completed C (P);
         if (ring == 1) {
            if ((rc = complete_columns (1, D.send_rows.data (), D.give.data (), D.halo_rows.data (), D.n_halo, C))) return rc;
            install_completed_halo (C);
         } else {
            // a ring that came out empty everywhere ends the selection
            std::vector<int64_t> all (P + 1, 0);
            if (comm->allgather_i64_host (comm->ctx, got, all.data ())) return fail (NKP_ECOMM, "nkp_create_dist: allgather failed");
            if (!std::any_of (all.begin (), all.begin () + P, [] (int64_t n) { return n != 0; })) break;
            std::vector<int32_t> wanted, req;
            std::vector<int> req_give;
            if ((rc = request_ring (ring, wanted, req, req_give))) return rc;
            if ((rc = complete_columns (ring, req.data (), req_give.data (), wanted.data (), (int64_t) wanted.size () - 1, C))) return rc;
         }
         const size_t before = ocols.size ();
         if ((rc = select_and_fetch (ring, C, &got))) return rc;
         int64_t announced = 0;
         for (size_t c = before; c < ocols.size (); c++) announced += ocols[c].len;
         rc = got == announced ? NKP_OK : fail (NKP_ECOMM, ring == 1 ? "nkp_create_dist: overlap rows announced and received differ" : "nkp_create_dist: ring rows announced and received differ");
         if ((rc = agree (rc, ring == 1 ? "overlap rows" : "ring rows"))) return rc;
         n_sel_all += got;
         ring_first.push_back ((int) arr_gid.size ());
      }
      return NKP_OK;
   }

   // ---- step 4: the matrix of the hierarchy -- own rows, then the overlap rows in ascending global row order (grouped by owner,
   // so that an exchange lands them in place); columns renumbered, couplings that leave [own | overlap] dropped
   void assemble ()
   {
      std::vector<size_t> cord (ocols.size ());
      for (size_t c = 0; c < cord.size (); c++) cord[c] = c;
      std::sort (cord.begin (), cord.end (), [&] (size_t a, size_t b) { return ocols[a].g0 < ocols[b].g0; });
      D.e_blk.assign (blk_start_loc, blk_start_loc + nblk_loc + 1);
      D.e_ci.assign (o.col_i, o.col_i + nblk_loc);
      D.e_cj.assign (o.col_j, o.col_j + nblk_loc);
      {
         const int64_t per = (coupled_tracer_cnt > 1 && nblk_loc % coupled_tracer_cnt == 0) ? nblk_loc / coupled_tracer_cnt : nblk_loc;
         D.e_ct.resize ((size_t) nblk_loc);
         for (int64_t c = 0; c < nblk_loc; c++) D.e_ct[(size_t) c] = o.col_t ? o.col_t[c] : (int32_t) (c / per);
      }
      std::vector<int32_t> ov_gid, ov_ecol, ov_ring;          // per overlap row (hierarchy order): global id, its column in e_*, ring
      std::vector<int64_t> ov_arr;                            // its arrived row
      const auto hbeg = D.halo_rows.begin (), hend = D.halo_rows.begin () + D.n_halo;
      for (size_t k = 0; k < cord.size (); k++) {
         const OvCol &c = ocols[cord[k]];
         for (int t = 0; t < c.len; t++) {
            ov_gid.push_back (arr_gid[(size_t) (c.row0 + t)]);
            ov_arr.push_back (c.row0 + t);
            ov_ecol.push_back ((int32_t) D.e_ci.size ());
            ov_ring.push_back (c.ring);
            const auto it = std::lower_bound (hbeg, hend, ov_gid.back ());
            D.sel_hpos.push_back ((it != hend && *it == ov_gid.back ()) ? (int32_t) (it - hbeg) : -1);
         }
         D.n_sel += c.len;
         D.e_blk.push_back ((int32_t) (m_loc + D.n_sel));
         D.e_ci.push_back (c.ci);
         D.e_cj.push_back (c.cj);
         D.e_ct.push_back (0);
      }
      const int64_t n_sel = D.n_sel;
      auto ext_of_global = [&] (int64_t g) -> int64_t {
         if (owned (g)) return g - fst_row;
         const auto it = std::lower_bound (ov_gid.begin (), ov_gid.end (), (int32_t) g);
         if (it == ov_gid.end () || *it != (int32_t) g) return -1;
         return m_loc + (it - ov_gid.begin ());
      };
      const int64_t n_eent = (int64_t) arr_col.size ();
      D.e_rowptr.assign ((size_t) (m_loc + n_sel) + 1, 0);
      D.e_colind.reserve ((size_t) (nnz_loc + n_eent));
      D.e_val.reserve ((size_t) (nnz_loc + n_eent));
      D.e_org.reserve ((size_t) (nnz_loc + n_eent));
      // (column, value, origin); columns are unique within a row, so the sort puts the origins where it puts the values
      struct Ent { int32_t col; double v; int32_t org; };
      std::vector<Ent> rowbuf;
      auto flush_row = [&] (int64_t r) {
         bool sorted = true;
         for (size_t k = 1; k < rowbuf.size () && sorted; k++) sorted = rowbuf[k].col > rowbuf[k - 1].col;
         if (!sorted) std::sort (rowbuf.begin (), rowbuf.end (), [] (const Ent &a, const Ent &b) { return a.col < b.col; });
         for (const Ent &pr : rowbuf) { D.e_colind.push_back (pr.col); D.e_val.push_back (pr.v); D.e_org.push_back (pr.org); }
         D.e_rowptr[(size_t) r + 1] = (int32_t) D.e_colind.size ();
         rowbuf.clear ();
      };
      for (int64_t r = 0; r < m_loc; r++) {
         for (int e = rowptr_loc[r]; e < rowptr_loc[r + 1]; e++) {
            const int32_t x = D.colind_ext[(size_t) e];
            if (x < m_loc) rowbuf.push_back ({ x, val[e], (int32_t) e });
            else {
               const int64_t q = ext_of_global (colind_glob[e]);
               if (q >= 0) {
                  rowbuf.push_back ({ (int32_t) q, val[e], (int32_t) e });
                  D.e_ct[(size_t) ov_ecol[(size_t) (q - m_loc)]] = D.e_ct[(size_t) col_of[(size_t) r]];   // an overlap column carries the tracer of the rows that see it
               }
            }
         }
         flush_row (r);
      }
      // ... and a column of ring k + 1 that of the rows of ring k
      for (int ring = 1; ring < rings; ring++)
         for (int64_t k = 0; k < n_sel; k++) {
            if (ov_ring[(size_t) k] != ring) continue;
            for (int64_t e = arr_ptr[(size_t) ov_arr[(size_t) k]]; e < arr_ptr[(size_t) ov_arr[(size_t) k] + 1]; e++) {
               const int64_t q = ext_of_global (arr_col[(size_t) e]);
               if (q >= m_loc && ov_ring[(size_t) (q - m_loc)] == ring + 1) D.e_ct[(size_t) ov_ecol[(size_t) (q - m_loc)]] = D.e_ct[(size_t) ov_ecol[(size_t) k]];
            }
         }
      // overlap rows; an entry's origin is its position in the value stream of all overlap rows in this order, which is the
      // order the owners ship them in (ascending rows per destination)
      D.ent_need.assign (P, 0);
      D.ras_need.assign (P, 0);
      int64_t q = 0;
      int p = 0;
      for (int64_t k = 0; k < n_sel; k++) {
         while (ov_gid[(size_t) k] >= starts[(size_t) p + 1]) p++;
         const int64_t a = ov_arr[(size_t) k];
         for (int64_t e = arr_ptr[(size_t) a]; e < arr_ptr[(size_t) a + 1]; e++, q++) {
            const int64_t x = ext_of_global (arr_col[(size_t) e]);
            if (x < 0) continue;
            rowbuf.push_back ({ (int32_t) x, arr_val[(size_t) e], (int32_t) (-1 - q) });
         }
         D.ent_need[p] += (int) (arr_ptr[(size_t) a + 1] - arr_ptr[(size_t) a]);
         D.ras_need[p]++;
         flush_row (m_loc + k);
      }
      ov_need = D.ras_need;
   }

   // ---- step 6: the fine-level exchange, per colour of the water columns.  Nothing new is asked of the peers: what this rank
   // shipped (step 3) is what its peers hold as overlap rows, and the overlap columns carry their grid positions (step 4), so
   // both sides split the same rows by the same colours.  An owner's rows reach a peer ascending, which is the hierarchy's
   // order of that peer's overlap rows (ascending global rows, grouped by owner)
   void smooth_lists ()
   {
      D.smooth = (D.ras && smooth) ? 1 : 0;
      if (!D.smooth) return;                                          // (every list stays empty)
      for (int c = 0; c < 2; c++) {
         D.smooth_give[c].assign (P, 0);
         D.smooth_need[c].assign (P, 0);
      }
      for (int p = 0; p < P; p++)
         for (int32_t r : shipped[(size_t) p]) {                      // (sorted by record_shipping)
            const int32_t col = col_of[(size_t) r];
            const int c = (o.col_i[col] + o.col_j[col]) & 1;
            D.smooth_send_rows[c].push_back (r);
            D.smooth_give[c][p]++;
         }
      int p = 0;
      int64_t left = ov_need.empty () ? 0 : ov_need[0];
      for (size_t ec = (size_t) nblk_loc; ec + 1 < D.e_blk.size (); ec++) {
         const int c = (D.e_ci[ec] + D.e_cj[ec]) & 1;
         for (int32_t r = D.e_blk[ec]; r < D.e_blk[ec + 1]; r++) {
            while (left == 0 && p + 1 < P) left = ov_need[(size_t) ++p];
            left--;
            D.smooth_recv_rows[c].push_back (r);
            D.smooth_need[c][p]++;
         }
      }
   }

   // ---- step 5: what the owner ships over all rings, ascending rows per destination: the entries (for nkp_refactor_dist) and,
   // with two or more rings, the rows of the residual exchange (one ring: the overlap residual is read from the SpMV halo)
   int record_shipping ()
   {
      D.ent_give.assign (P, 0);
      D.ras_give.assign (P, 0);
      int64_t ent_total = 0, recv_total = 0;
      for (int p = 0; p < P; p++) {
         std::vector<int32_t> &rows = shipped[(size_t) p];
         std::sort (rows.begin (), rows.end ());
         for (int32_t r : rows) {
            for (int e = rowptr_loc[r]; e < rowptr_loc[r + 1]; e++) D.ship_e.push_back ((int32_t) e);
            D.ent_give[p] += rowptr_loc[r + 1] - rowptr_loc[r];
            D.ras_send_rows.push_back (r);
         }
         D.ras_give[p] = (int) rows.size ();
         ent_total += D.ent_give[p];
         recv_total += D.ent_need[p];
      }
      if (rings >= 2) {
         int rc = D.n_sel != n_sel_all ? fail (NKP_ECOMM, "nkp_create_dist: overlap rows announced and received differ")
                  : std::max (ent_total, recv_total) >= 2147483647LL ? fail (NKP_EINVAL, "nkp_create_dist: overlap rows of all rings exceed the int32 exchange counts") : NKP_OK;
         if ((rc = agree (rc, "overlap rows of all rings"))) return rc;
      } else {
         D.ras_send_rows.clear ();
         D.ras_need.clear ();
         D.ras_give.clear ();
      }
      // overlap is worth its exchange only if some rank has any: same decision everywhere
      std::vector<int64_t> all (P + 1, 0);
      if (comm->allgather_i64_host (comm->ctx, D.n_sel, all.data ())) return fail (NKP_ECOMM, "nkp_create_dist: allgather failed");
      for (int p = 0; p < P; p++) D.ras = D.ras || all[p] > 0;
      D.rings = D.ras ? (int) rings : 0;
      smooth_lists ();                                        // 6. the fine-level exchange, if the ranks agreed on it
      return NKP_OK;
   }
};

}   // namespace

// Restricted additive Schwarz (overlap of rings of water columns).  A hierarchy built from the rank's diagonal block alone
// treats the cut through the ocean as a wall: latitude bands cost 2-3 times the iterations of the undivided solve (1 degree:
// 78 / 157 / 238 for 1 / 2 / 4 bands), and a global coarsest level does not repair that (scipy prototype tools/proto_bands.py:
// 36 / 58 / 89 without, 57 / 87 with it).  What does is the classical remedy: every rank's hierarchy also covers the water
// columns of other ranks that its own rows couple to LATERALLY (the halo of the SpMV, completed to whole columns), a cycle runs
// on [own rows | overlap rows] with the residual of the overlap rows fetched from their owners, and only the own part of the
// result is kept (prototype: 36 / 43 / 55).  Columns of OTHER TRACERS at a cell this rank owns are not overlap (a
// tracer-per-rank partition keeps its block-Jacobi preconditioner): a halo column joins only if its (i, j) is not the position
// of an own column.  dist_ras_rings > 1 deepens the overlap ring by ring (prototype, 3 degrees, 4 bands: 63 / 56 / 53 / 51
// iterations for 1-4 rings); each ring is one more round of complete / select / fetch.
int dist_plan (DistPlan &D, const nkp_comm_ops *comm, const nkp_options &o, const std::vector<int64_t> &starts, int64_t fst_row, int64_t m_loc,
               int64_t nnz_loc, const int32_t *rowptr_loc, const int32_t *colind_glob, const double *val, const int32_t *blk_start_loc,
               int64_t nblk_loc, int coupled_tracer_cnt)
{
   Planner pl = { D, comm, o, starts, fst_row, m_loc, nnz_loc, rowptr_loc, colind_glob, val, blk_start_loc, nblk_loc, coupled_tracer_cnt };
   int rc;
   if ((rc = pl.spmv_halo ())) return rc;                  // 1. SpMV halo and send lists
   if ((rc = pl.agree_on_depth ())) return rc;             // 2. the overlap depth of all ranks
   if (pl.rings <= 0) return NKP_OK;
   if ((rc = pl.fetch_rings ())) return rc;                // 3. ring by ring: complete, select, fetch
   pl.assemble ();                                         // 4. the hierarchy's source matrix and its value origins
   return pl.record_shipping ();                           // 5. what the owner ships; does any rank have overlap?
}

struct nkp_dist_plan { DistPlan D; int nranks = 0; int64_t m_loc = 0, nnz_loc = 0; };

extern "C" int nkp_dist_overlap_plan_host (nkp_dist_plan **out, const nkp_options *opt, int64_t n_global, int64_t fst_row, int64_t m_loc, int64_t nnz_loc,
                                           const int32_t *rowptr_loc, const int32_t *colind_glob, const double *val, const int32_t *blk_start_loc,
                                           int64_t nblk_loc, int coupled_tracer_cnt, const nkp_comm_ops *comm)
{
   if (!out || !comm || !rowptr_loc || !comm->alltoallv_i32_host || !comm->allgather_i64_host) return fail (NKP_EINVAL, "nkp_dist_overlap_plan_host: bad arguments");
   *out = nullptr;
   const int P = comm->nranks;
   std::vector<int64_t> starts (P + 1, 0);
   if (comm->allgather_i64_host (comm->ctx, fst_row, starts.data ())) return fail (NKP_ECOMM, "nkp_dist_overlap_plan_host: allgather failed");
   starts[P] = n_global;
   nkp_options o;
   if (opt) o = *opt;
   else nkp_default_options (&o);
   nkp_dist_plan *pl = new nkp_dist_plan;
   pl->nranks = P;
   pl->m_loc = m_loc;
   pl->nnz_loc = nnz_loc;
   const int rc = dist_plan (pl->D, comm, o, starts, fst_row, m_loc, nnz_loc, rowptr_loc, colind_glob, val, blk_start_loc, nblk_loc, coupled_tracer_cnt);
   if (rc) { delete pl; return rc; }
   *out = pl;
   return NKP_OK;
}

// one table for sizes and copies: name -> (pointer, element count, element size)
static bool dist_plan_field (const nkp_dist_plan *p, const char *what, const void **ptr, int64_t *count, size_t *elem)
{
   const DistPlan &D = p->D;
   const int64_t n_ext = p->m_loc + D.n_sel;
   struct F { const char *name; const void *ptr; int64_t count; size_t elem; };
   const F fields[] = {
      { "colind_ext", D.colind_ext.data (), p->nnz_loc, 4 }, { "halo_rows", D.halo_rows.data (), D.n_halo, 4 }, { "send_rows", D.send_rows.data (), D.nsend, 4 },
      { "need", D.need.data (), p->nranks, 4 }, { "give", D.give.data (), p->nranks, 4 },
      { "rowptr", D.e_rowptr.data (), D.e_rowptr.empty () ? 0 : n_ext + 1, 4 }, { "colind", D.e_colind.data (), (int64_t) D.e_colind.size (), 4 },
      { "val", D.e_val.data (), (int64_t) D.e_val.size (), 8 }, { "blk_start", D.e_blk.data (), (int64_t) D.e_blk.size (), 4 },
      { "col_i", D.e_ci.data (), (int64_t) D.e_ci.size (), 4 }, { "col_j", D.e_cj.data (), (int64_t) D.e_cj.size (), 4 }, { "col_t", D.e_ct.data (), (int64_t) D.e_ct.size (), 4 },
      { "sel_hpos", D.sel_hpos.data (), D.n_sel, 4 },
      { "ras_send_rows", D.ras_send_rows.data (), (int64_t) D.ras_send_rows.size (), 4 }, { "ras_need", D.ras_need.data (), (int64_t) D.ras_need.size (), 4 },
      { "ras_give", D.ras_give.data (), (int64_t) D.ras_give.size (), 4 },
      { "origin", D.e_org.data (), (int64_t) D.e_org.size (), 4 }, { "ship", D.ship_e.data (), (int64_t) D.ship_e.size (), 4 },
      { "ent_give", D.ent_give.data (), (int64_t) D.ent_give.size (), 4 }, { "ent_need", D.ent_need.data (), (int64_t) D.ent_need.size (), 4 },
      { "smooth_send_rows0", D.smooth_send_rows[0].data (), (int64_t) D.smooth_send_rows[0].size (), 4 },
      { "smooth_send_rows1", D.smooth_send_rows[1].data (), (int64_t) D.smooth_send_rows[1].size (), 4 },
      { "smooth_recv_rows0", D.smooth_recv_rows[0].data (), (int64_t) D.smooth_recv_rows[0].size (), 4 },
      { "smooth_recv_rows1", D.smooth_recv_rows[1].data (), (int64_t) D.smooth_recv_rows[1].size (), 4 },
      { "smooth_give0", D.smooth_give[0].data (), (int64_t) D.smooth_give[0].size (), 4 }, { "smooth_give1", D.smooth_give[1].data (), (int64_t) D.smooth_give[1].size (), 4 },
      { "smooth_need0", D.smooth_need[0].data (), (int64_t) D.smooth_need[0].size (), 4 }, { "smooth_need1", D.smooth_need[1].data (), (int64_t) D.smooth_need[1].size (), 4 },
   };
   for (const F &f : fields)
      if (!strcmp (what, f.name)) { *ptr = f.ptr; *count = f.count; *elem = f.elem; return true; }
   return false;
}

extern "C" int64_t nkp_dist_plan_size (const nkp_dist_plan *p, const char *what)
{
   if (!p || !what) return -1;
   if (!strcmp (what, "ras")) return p->D.ras ? 1 : 0;
   if (!strcmp (what, "n_sel")) return p->D.n_sel;
   if (!strcmp (what, "n_halo")) return p->D.n_halo;
   if (!strcmp (what, "ras_rings")) return p->D.rings;
   if (!strcmp (what, "smooth_exchange")) return p->D.smooth;
   const void *ptr; int64_t count; size_t elem;
   return dist_plan_field (p, what, &ptr, &count, &elem) ? count : -1;
}

extern "C" int nkp_dist_plan_copy (const nkp_dist_plan *p, const char *what, void *dst)
{
   const void *ptr; int64_t count; size_t elem;
   if (!p || !what || !dst || !dist_plan_field (p, what, &ptr, &count, &elem)) return fail (NKP_EINVAL, "nkp_dist_plan_copy: unknown field");
   if (count > 0) memcpy (dst, ptr, (size_t) count * elem);
   return NKP_OK;
}

extern "C" void nkp_dist_plan_free (nkp_dist_plan *p) { delete p; }

// ---------------------------------------------------------------- cell-major partition (host only)
extern "C" int nkp_cell_major_order (int64_t nblk, const int32_t *blk_start, int cnt, int32_t *perm, int32_t *blk_start_new, int32_t *col_t, int32_t *col_src)
{
   if (!blk_start || !perm || !blk_start_new || !col_t || !col_src || cnt < 1 || nblk < 0 || nblk % cnt != 0)
      return fail (NKP_EINVAL, "nkp_cell_major_order: bad arguments (nblk = %lld must be a multiple of the tracer count %d)", (long long) nblk, cnt);
   const int64_t per = nblk / cnt;
   for (int t = 1; t < cnt; t++)
      for (int64_t c = 0; c <= per; c++)
         if (blk_start[t * per + c] - blk_start[t * per] != blk_start[c] - blk_start[0])
            return fail (NKP_EINVAL, "nkp_cell_major_order: tracer %d does not have the water columns of tracer 0 (block %lld)", t, (long long) c);
   int64_t row = 0, b = 0;
   blk_start_new[0] = 0;
   for (int64_t c = 0; c < per; c++)
      for (int t = 0; t < cnt; t++, b++) {
         const int64_t old = t * per + c;
         for (int r = blk_start[old]; r < blk_start[old + 1]; r++) perm[row++] = r;
         blk_start_new[b + 1] = (int32_t) row;
         col_t[b] = t;
         col_src[b] = (int32_t) old;
      }
   return NKP_OK;
}

extern "C" int nkp_permuted_rows (int64_t n, const int32_t *rowptr, const int32_t *colind, const double *val, const int32_t *perm, const int32_t *inv,
                                  int64_t r0, int64_t r1, int32_t *rowptr_loc, int32_t *colind_loc, double *val_loc)
{
   if (!rowptr || !perm || !inv || !rowptr_loc || r0 < 0 || r1 < r0 || r1 > n) return fail (NKP_EINVAL, "nkp_permuted_rows: bad arguments");
   rowptr_loc[0] = 0;
   for (int64_t r = r0; r < r1; r++) {
      const int old = perm[r];
      rowptr_loc[r - r0 + 1] = rowptr_loc[r - r0] + (rowptr[old + 1] - rowptr[old]);
   }
   const int nt = (r1 - r0 >= 200000) ? (int) std::min (16u, std::max (1u, std::thread::hardware_concurrency ())) : 1;
   auto work = [&] (int t) {
      std::vector<std::pair<int32_t, double>> buf;
      const int64_t a = r0 + (r1 - r0) * t / nt, b = r0 + (r1 - r0) * (t + 1) / nt;
      for (int64_t r = a; r < b; r++) {
         const int old = perm[r];
         buf.clear ();
         for (int e = rowptr[old]; e < rowptr[old + 1]; e++) buf.push_back ({ inv[colind[e]], val[e] });
         std::sort (buf.begin (), buf.end (), [] (const std::pair<int32_t, double> &x, const std::pair<int32_t, double> &y) { return x.first < y.first; });
         int64_t o = rowptr_loc[r - r0];
         for (const auto &pr : buf) { colind_loc[o] = pr.first; val_loc[o] = pr.second; o++; }
      }
   };
   if (nt == 1) work (0);
   else {
      std::vector<std::thread> pool;
      for (int t = 0; t < nt; t++) pool.emplace_back (work, t);
      for (std::thread &th : pool) th.join ();
   }
   return NKP_OK;
}
