// New matrix values on an existing solver's pattern (nkp_refactor, refactor.hip): the value passes of the hierarchy on the
// device, with the maps that tie every value to the slot the setup gave it.  Not part of the C ABI.  The entry points and the
// order these passes run in are refactor_api.hip.
#pragma once
#include "multilevel.h"
#include "nkp_dev.h"

#include <vector>

struct RefactorWork {
   double *aval = nullptr;       // [nnz + 2] staged new values of A (written before anything a solve reads)
   int *dcnt = nullptr;          // [4 + 2 * levels] device counters: pattern drift, rows without a (non-zero) diagonal, first such row + 1, -, factor status per level
   size_t bytes = 0;             // device bytes of everything below (counted in the solver's device_bytes)
   bool maps = false;            // the maps below exist (first fast-path refactor)
   int *tslot = nullptr;         // [nnz of A] colour-major slot s of the entry's twin value in level 0: s between water columns and on the
                                 // diagonal, -2 - s inside a column, -1 = dropped
   struct Lev {
      double *nv = nullptr;      // [nnz] new f64 values, colour-major
      int *gptr = nullptr, *gidx = nullptr;   // this level's entries as sums of the previous level's: slot -> fine entries (levels >= 1)
      int nph = 0;               // coarse pairs the setup dropped as exact zeros ...
      int *pptr = nullptr, *pidx = nullptr;   // ... and their fine entries
      int *gcols = nullptr;      // columns of every lane group (sorted-group lane layouts only)
   };
   std::vector<Lev> lev;
   int *col_gcols = nullptr;     // same for the column preconditioner's blocks
   bool col_gcols_done = false;
   std::vector<int> last_rowptr, last_colind;   // host pattern of the coarsest level (dense inverse)
   double *inv_new = nullptr;    // coarsest inverse of the new values, computed before the commit point
   float *invf_new = nullptr;
   int ldf_new = 0;
   size_t inv_bytes = 0;
   int inv_pivoted = 0;          // ml_coarse_inverse's return value for inv_new: 1 = the pivoted routine made it
};

// free the maps (keeps aval / dcnt); returns the bytes released
size_t rf_free_maps (RefactorWork &W);
void rf_free (RefactorWork &W);
// staging buffers for n rows / nnz entries and nlev levels; 0 or -2
int rf_stage (RefactorWork &W, int64_t nnz, int nlev);
// rows of A (natural order, values in W.aval) with no non-zero diagonal: count into W.dcnt[1], first row + 1 into W.dcnt[2]
void rf_launch_diag_check (const CsrDev &A, const double *val, int *dcnt, hipStream_t st);
// R_i = 1 / max_j |a_ij|, R_i^-1 (the host loop of nkp_create), rows without entries keep 1
void rf_launch_row_scale (const CsrDev &A, const double *val, double *rscale, double *rinv, hipStream_t st);
// the maps of the fast path (host work + uploads, once per hierarchy); 0, -2 (no memory), -3 (HIP failure), 1 (the hierarchy is
// not one the fast path covers)
int rf_build_maps (RefactorWork &W, const MlHierarchy &H, const CsrDev &A, hipStream_t st);
// twin and Galerkin values of every level from the values val of A (the matrix the hierarchy was built from) into
// W.lev[l].nv; pattern drift counted into W.dcnt[0] (enqueued only)
void rf_values (RefactorWork &W, const MlHierarchy &H, const CsrDev &A, const double *val, hipStream_t st);
// dense inverse of the new coarsest operator into W.inv_new / invf_new (before the commit point); 0, -4 (singular), -2 / -3
int rf_prepare_inverse (RefactorWork &W, const MlHierarchy &H, hipStream_t st, char *err, size_t errlen);
// the prepared inverse fits the buffers the hierarchy (and its clones) point at
bool rf_inverse_same_storage (const RefactorWork &W, const MlHierarchy &H);
void rf_drop_inverse (RefactorWork &W);
// commit the new values: f64 / f32 operators, column factors and their lane layouts, coarsest inverse.  0, -4 (zero pivot or
// -2 / -3; *replaced = 1 if the prepared coarsest inverse needed buffers of another shape (pointers changed)
int rf_commit (RefactorWork &W, MlHierarchy &H, hipStream_t st, char *err, size_t errlen, int *replaced);
// column-block preconditioner: factors of A (new values already in A.val) + their lane layout; 0 or -4 (zero pivot, row in err)
int rf_column_factor (RefactorWork &W, const CsrDev &A, ColBlocksDev &B, hipStream_t st, char *err, size_t errlen);

// nkp_refactor_dist (refactor_dist.hip): where every value of a distributed rank's hierarchy source comes from.  The source is
// the diagonal block (no overlap) or the [own rows | overlap rows] matrix of restricted additive Schwarz; nkp_create_dist keeps
// this plan in host memory, the first nkp_refactor_dist uploads it.
struct DistRefactorPlan {
   int64_t n_src = 0, nnz_src = 0;               // rows / entries of the hierarchy's source matrix
   std::vector<int32_t> src_rowptr, src_colind;  // its pattern on the host until the first refactor uploads it (then read back)
   std::vector<int32_t> origin;                  // [nnz_src] >= 0: own local entry e (caller's order); < 0: -1 - position in the received overlap values
   std::vector<int32_t> ship;                    // own local entries of the overlap rows this rank ships, in shipping order
   std::vector<int> ship_counts, recv_counts;    // values per rank sent / received (restricted additive Schwarz only)
   int64_t n_recv = 0;
   bool exchange = false;                        // the source has overlap rows somewhere: every rank takes part in the value exchange
   // device, from the first nkp_refactor_dist on
   bool uploaded = false;
   CsrDev src;                                   // pattern of the source (val unused)
   double *sval = nullptr;                       // [nnz_src] its new values
   double *sendbuf = nullptr, *recvbuf = nullptr;
   int *d_origin = nullptr, *d_ship = nullptr;
   size_t bytes = 0;                             // device bytes of the above (counted in the solver's device_bytes)
};

// device copies of the plan; 0 or -2 (no memory) / -3 (HIP failure).  The host pattern is released once uploaded.
int rf_dist_upload (DistRefactorPlan &Q, hipStream_t st);
void rf_dist_free (DistRefactorPlan &Q);
// sendbuf[k] = aval[ship[k]]
void rf_dist_launch_pack (const DistRefactorPlan &Q, const double *aval, hipStream_t st);
// sval[k] = origin[k] >= 0 ? aval[origin[k]] : recvbuf[-1 - origin[k]]
void rf_dist_launch_assemble (const DistRefactorPlan &Q, const double *aval, hipStream_t st);
