// The solver object, and what the host-side units that work on it share.  Each of these units has one concern:
//   solver.hip          lifetime of the object, messages, stream, counters (nkp_destroy, nkp_set_stream, nkp_get_int)
//   create.hip          nkp_create, nkp_create64, nkp_clone: validation, uploads, work vectors, hierarchy, column factors
//   create_dist.hip     nkp_create_dist, nkp_gather_root (the host-side plan: dist_plan.cpp)
//   krylov.hip          one right-hand side: operator and preconditioner of a solve, FGMRES, BiCGStab, nkp_solve
//   krylov_host.cpp     the host arithmetic of FGMRES (krylov_host.h): no HIP, no solver object
//   batch_solve.hip     K right-hand sides in lockstep (nkp_solve_batch_device); the kernels are batch.hip
//   solve_controls.hip  rtol, atol and max_iters after creation (nkp_set_solve_controls) and per column (nkp_solve_batch_device_ex)
//   smooth_exchange.hip the fine-level exchange of a row-distributed cycle (tuning dist_smooth_exchange): kernels, lists, the cycle's hook
//   inspect.hip         entry points of tests and timing (arrays of the hierarchy and the matrix, single products, nkp_time_kernel)
//   refactor_api.hip, transpose*.hip, valgrad_api.hip, valprod_api.hip, valprod_trans_dist.hip      new values, A^T, gradient and products by values
//   residual_api.hip    residual, norms and backward error of K given solutions (nkp_residual_batch); the kernel is residual.hip
//   operand_call.h      what valgrad_api, valprod_api, valprod_trans_dist and residual_api share: the envelope of a K-vector call on the
//                       pattern (OperandCall: arguments, work space, the two agreements), column staging, Stopwatch, release_buffers
// What crosses units is declared once, below, under the unit that defines it.  Private to the library: nothing here is part of
// the C ABI.
#pragma once
#include "../../include/nkp.h"
#include "nkp_dev.h"
#include "multilevel.h"
#include "refactor.h"
#include "dist_plan.h"
#include "row_exchange.h"
#include "krylov_host.h"

#include <atomic>
#include <initializer_list>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#define HIPCHK(call)                                                                             \
   do {                                                                                          \
      hipError_t e_ = (call);                                                                    \
      if (e_ != hipSuccess) return fail (NKP_EDEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString (e_), __FILE__, __LINE__); \
   } while (0)

// The three values of a solve that may change after creation (nkp_set_solve_controls).  They live in nkp_solver::opt, where every
// driver reads them at the start of a solve; `created` keeps what nkp_create was given
struct SolveControls {
   int max_iters;
   double rtol, atol;
};

struct nkp_solver {
   nkp_options opt;
   SolveControls created = { 0, 0.0, 0.0 };
   nkp_tuning tune;             // resolved once in nkp_create; the matrix, column-block and hierarchy objects point at it
   int device = 0;
   bool stagnated = false;      // last solve stopped by the attainable-accuracy guard
   int rhs_class = 0;           // last solve's verdict on its right-hand side (RHS_* of krylov_host.h)
   bool borrowed = false;       // nkp_clone: matrix, factors and hierarchy belong to the solver this one was cloned from
   hipStream_t stream = nullptr;
   bool own_stream = false;
   CsrDev A;
   ColBlocksDev B;
   MlHierarchy ml;
   // row-distributed flavour: halo exchange before every SpMV, allreduce after every local reduction
   struct {
      bool on = false;
      nkp_comm_ops ops;
      int64_t n_global = 0, fst = 0, n_halo = 0;
      // the exchanges of rows between the ranks (row_exchange.h): each owns its index lists, counts and buffers; where the rows land
      // (xe, bxe, rext, sel_idx) is the solver's.  x_halo: the local rows other ranks read as columns, to behind the own rows of xe / bxe,
      // and the overlap residual of one ring; x_ras: that of more rings; x_smooth[c]: the fine-level exchange of colour c
      RowExchange x_halo, x_ras, x_smooth[2];
      template <class F> void each_exchange (F f) { f (x_halo, on); f (x_ras, ras_sep); f (x_smooth[0], smooth); f (x_smooth[1], smooth); }      // (exchange, in force)
      double *xe = nullptr;           // [n + n_halo] extended SpMV input: own rows then halo rows
      // overlap of the halo exchange with the SpMV of the interior rows (rows without off-rank columns): the row blocks
      // are built per segment [head boundary rows | interior | tail boundary rows]; seg_rb[q] = first row block of segment q
      int seg_rb[4] = { 0, 0, 0, 0 };
      bool overlap = false;
      hipStream_t comm_stream = nullptr;
      hipEvent_t ev_packed = nullptr, ev_halo = nullptr;
      // restricted additive Schwarz: the hierarchy of this rank also covers the neighbouring ranks' water columns its rows
      // couple to laterally (one ring); a cycle runs on [own rows | those halo rows] and only the own part is kept
      bool ras = false;
      int64_t n_ext = 0, n_sel = 0;
      int *sel_idx = nullptr;         // position in the halo of every overlap row (one ring)
      double *rext = nullptr, *zext = nullptr;
      // two or more rings (tuning dist_ras_rings): rows of ring 2 and beyond are not in the SpMV halo, so the overlap residual has
      // an exchange of its own (x_ras); the rows arrive at rext + n in the hierarchy's order, K wide in x_ras.brecv
      int ras_rings = 0;              // the depth the ranks agreed on, 0 without overlap
      bool ras_sep = false;
      // fine-level exchange (tuning dist_smooth_exchange; smooth_exchange.hip): after a level-0 half sweep of colour c the overlap
      // rows of that colour take their owners' x.  Per colour: the plan's rows in host memory (own local rows sent by destination;
      // overlap rows of the hierarchy's matrix in arrival order); x_smooth[c] has them as level-0 positions (rebuilt with perm0)
      bool smooth = false;
      MlSmoothHook smooth_hook = { nullptr, nullptr };
      std::vector<int32_t> h_smooth_send[2], h_smooth_recv[2];
      // K right-hand sides in lockstep: the K-interleaved operator input [own rows | halo rows] x K, the
      // K-wide buffers of the exchanges, and the group's Gram-Schmidt messages
      // gmsg = dots [K x (m + 2)] | second pass [K x (m + 2)] | norms [K] | 1 / norms [K], ghpin its pinned host mirror
      double *bxe = nullptr, *gmsg = nullptr, *ghpin = nullptr;
      int bK = 0;                     // width these buffers exist for
      int agreed_K = 0;               // widest interleave every rank is known to have buffers for
      // nkp_transpose_dist: what nkp_create_dist was given and planned, in host memory -- the first rows of all ranks, the global
      // rows of the halo, the own rows the peers hold as halo (x_halo.send_idx), the caller's OWN block offsets and grid positions
      // (with overlap h_blk / h_col_* hold the extended [own | overlap] arrays)
      std::vector<int64_t> starts;
      std::vector<int32_t> h_halo_rows, h_send_rows, own_blk, own_ci, own_cj, own_ct;
      bool own_has_blk = false;
      int own_tracer_cnt = 1;
   } dist;
   int64_t n = 0, ld = 0;
   int m = 0;
   // work vectors
   bool vf32 = false;              // Krylov basis stored as float (stride ld floats inside the V allocation)
   double *vcur = nullptr;         // f64 copy of the newest basis vector (input of the next preconditioner call)
   double *V = nullptr, *Z = nullptr, *w = nullptr, *r = nullptr, *x = nullptr, *b = nullptr, *t1 = nullptr, *t2 = nullptr;
   double *p1 = nullptr, *p2 = nullptr;   // scratch of the multi-step preconditioner (NKP_PRECOND_STEPS > 1)
   int precond_steps = 1;        // configured cycles per application
   int steps_now = 1;            // cycles per application of the running solve (the run-time guard may lower it for one solve)
   bool equil = false;           // row-weighted FGMRES
   double *rscale = nullptr, *rinv = nullptr;   // R and R^-1 (device), R_i = 1 / max_j |a_ij|
   double *eqtmp = nullptr;      // R^-1 v_j, the input of the preconditioner in the row-weighted iteration
   bool comm_failed = false;     // a collective callback returned non-zero: every verdict after that is NKP_ECOMM
   double *partial = nullptr;       // reduction scratch
   double *dscal = nullptr;         // device scalars: h[m+2] | h2[m+2] | misc[16] | ycoef[m+1]
   double *hpin = nullptr;          // pinned host mirror
   int *dint = nullptr;             // device ints
   // K right-hand sides at once (nkp_solve_batch_device): K - 1 more sets of work vectors (clones sharing this solver's stream)
   // and three K-interleaved vectors around the batched operator / cycle application
   std::vector<nkp_solver *> batch_members;
   double *bvin = nullptr, *bz = nullptr, *bw = nullptr;
   int batch_K = 0;
   int64_t batch_steps = 0;         // batched operator applications (lockstep Krylov steps) over the solver's life
   int batch_width = 0;             // K of the last batched group
   size_t device_bytes = 0;
   double create_seconds = 0.0;     // wall time of nkp_create
   // nkp_refactor: state shared by a solver and its clones (live clones, a refactor that failed after its commit point),
   // the owner's work space, and the host arrays a rebuild of the hierarchy needs again
   struct Shared {
      std::atomic<int> clones { 0 };
      std::atomic<int64_t> alltoallv_calls { 0 }, allreduce_calls { 0 };      // device collectives of solves (a batch's members count here too)
      bool broken = false;
      std::string why;
   };
   std::shared_ptr<Shared> shared = std::make_shared<Shared> ();
   RefactorWork *rf = nullptr;
   std::vector<int> h_blk, h_col_i, h_col_j, h_col_t;
   int tracer_cnt = 1;
   int64_t refactor_count = 0;
   int refactor_rebuilt = 0;
   double refactor_seconds = 0.0;
   // nkp_refactor_dist: where the values of the hierarchy's source come from (kept by nkp_create_dist, multilevel only)
   DistRefactorPlan *dplan = nullptr;
   int64_t refactor_halo_values = 0;
   // nkp_transpose: the solver of A^T this one owns (trans), or the solver this one was transposed from (trans_of); the owner
   // keeps the value map valT[p] = val[trans_src[p]] and, from its first refactor on, the gathered values (both on the device)
   nkp_solver *trans = nullptr, *trans_of = nullptr;
   int *trans_src = nullptr;
   double *trans_val = nullptr;
   size_t trans_map_bytes = 0;
   double trans_seconds = 0.0, trans_kernel_seconds = 0.0;
   // nkp_transpose_dist: trans_src[p] is then the origin of A^T's row block entry p -- a position in val, or -1 - position in the
   // received values; trans_ship = the positions in val of the entries shipped (grouped by destination), the entry counts per
   // rank, and, from the first refactor on, the send / receive buffers of the value exchange
   int *trans_ship = nullptr;
   double *trans_send = nullptr, *trans_recv = nullptr;
   std::vector<int> trans_send_counts, trans_recv_counts;
   int64_t trans_nnz = 0, trans_sent = 0, trans_received = 0;
   // nkp_value_gradient: the K-interleaved copies of lambda and x, the device staging of the host flavour (lambda and x side by
   // side, the gradient), each with its capacity in doubles -- made at first use, kept, counted in device_bytes
   struct {
      double *lam = nullptr, *x = nullptr, *stage = nullptr, *g = nullptr;
      size_t lam_cap = 0, x_cap = 0, stage_cap = 0, g_cap = 0;
      int64_t calls = 0;
      double seconds = 0.0;        // wall time of the last call
   } vg;
   // nkp_values_product / nkp_solve_tangent_device: the K-interleaved copy of x (single-GPU, nrhs >= 2), the device staging of the
   // host flavour (val | x | y), the right-hand sides R = dB - dA X of a tangent solve -- like vg made at first use and kept
   struct {
      double *x = nullptr, *stage = nullptr, *r = nullptr;
      size_t x_cap = 0, stage_cap = 0, r_cap = 0;
      int64_t calls = 0, tangent_calls = 0;
      double seconds = 0.0;        // wall time of the last product
   } vp;
   // nkp_values_product_trans: the pattern of A^T as an index, no values and no solver -- T.rowptr [n + 1], T.colind [nnz], T.rowblk
   // (the row blocks a solver created from the host transpose has) and src [nnz]: entry p of A^T takes its value from val[src[p]].
   // Built at the first call that needs it, all four arrays or none, kept (a refactor keeps the pattern), counted in device_bytes.
   // The owner's own: independent of trans / trans_src; a clone or a transposed handle never has one
   struct {
      CsrDev T;
      int *src = nullptr;
      size_t bytes = 0;
      double build_seconds = 0.0;
      int64_t calls = 0;
      double seconds = 0.0;        // wall time of the last product
      // nkp_values_product_trans_dist on a row-distributed solver (valprod_trans_dist.hip): T is then the row block of A^T this rank
      // assembles -- T.rowptr [m_loc + 1] and its row blocks, T.colind the x row of every assembled entry (a local row, or m_loc + q
      // for the q-th received product) -- and src its origin (a position in val_loc, or -1 - q).  The ship list (position in val_loc
      // and local row of every entry in a halo column, grouped by destination), the entries per rank, and the work space
      // xe = [ own rows | received products ] x K and the K-wide send buffer, grown when a wider K comes
      int *ship_e = nullptr, *ship_i = nullptr;
      int64_t n_ship = 0, n_recv = 0;
      std::vector<int> send_entries, recv_entries, send_k, recv_k;      // per rank; times the K of the last call
      double *xe = nullptr, *send = nullptr;
      size_t xe_cap = 0, send_cap = 0;
   } vt;
   // nkp_residual_batch: the K-interleaved copy of X (single-GPU, nrhs >= 2), the partials of the reductions (3 K doubles per row
   // block of A, the 3 K results behind them), the device staging of the host flavour (B | X | R) -- like vp made at first use and kept
   struct {
      double *x = nullptr, *partial = nullptr, *stage = nullptr;
      size_t x_cap = 0, partial_cap = 0, stage_cap = 0;
      int64_t calls = 0;
      double seconds = 0.0;        // wall time of the last call
   } rb;
   double *h_dev () { return dscal; }
   double *h2_dev () { return dscal + (m + 2); }
   double *misc_dev () { return dscal + 2 * (m + 2); }     // [0]=nrm2 [1]=inv [2]=dot out ...
   double *y_dev () { return dscal + 2 * (m + 2) + 16; }
};

template <class T>
static int dev_alloc (nkp_solver *s, T **p, size_t count)
{
   void *q = nullptr;
   size_t bytes = (count ? count : 1) * sizeof (T);
   hipError_t e = hipMalloc (&q, bytes);
   if (e != hipSuccess) return fail (NKP_ENOMEM, "hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString (e));
   *p = (T *) q;
   s->device_bytes += bytes;
   return NKP_OK;
}


// ---- work space made at first use (nkp_value_gradient, nkp_values_product) -----------------------------------------------------
struct Want {
   double **p;
   size_t *cap;        // doubles *p holds
   size_t need;        // doubles this call needs
};

// Grow the buffers of `set` that are too small, all of them or none: the new ones are allocated first and take the place of
// the old ones only when every allocation succeeded.  After a failure the solver holds exactly what it held before and HIP's
// last error is cleared.
inline int reserve (nkp_solver *s, std::initializer_list<Want> set, const char *who)
{
   double *fresh[8] = {};
   int rc = NKP_OK;
   size_t i = 0;
   for (const Want &w : set) {
      if (w.need > *w.cap) {
         void *q = nullptr;
         if (hipMalloc (&q, w.need * sizeof (double)) != hipSuccess) {
            rc = fail (NKP_ENOMEM, "%s: hipMalloc of %zu bytes of work space failed", who, w.need * sizeof (double));
            break;
         }
         fresh[i] = (double *) q;
      }
      i++;
   }
   if (rc) {
      for (double *q : fresh)
         if (q) (void) hipFree (q);
      (void) hipGetLastError ();
      return rc;
   }
   i = 0;
   for (const Want &w : set) {
      if (fresh[i]) {
         if (*w.p) {
            (void) hipFree (*w.p);
            s->device_bytes -= *w.cap * sizeof (double);
         }
         *w.p = fresh[i];
         *w.cap = w.need;
         s->device_bytes += w.need * sizeof (double);
      }
      i++;
   }
   return NKP_OK;
}

// the interleave width that serves nrhs vectors
inline int width_of (int nrhs) { return nrhs <= 1 ? 1 : nrhs <= 2 ? 2 : nrhs <= 4 ? 4 : 8; }

// the two device collectives of a solve; a failure leaves stale data behind and is checked before any verdict is returned
// (inline: they run on every Krylov step).  sticky = false: the caller reports the failure itself (fetch_x_operand)
inline int alltoallv_dev (nkp_solver *s, const double *send, const int *send_counts, double *recv, const int *recv_counts, hipStream_t st, bool sticky = true)
{
   s->shared->alltoallv_calls++;
   const int rc = s->dist.ops.alltoallv (s->dist.ops.ctx, send, send_counts, recv, recv_counts, (void *) st);
   if (rc && sticky) s->comm_failed = true;
   return rc;
}
// ONE alltoallv, always made and counted: the rows of exchange X, K wide in `packed`, arrive at `dest` on their receivers
inline int exchange_rows (nkp_solver *s, RowExchange &X, int K, const double *packed, double *dest, hipStream_t st, bool sticky = true)
{ return alltoallv_dev (s, packed, X.send_counts_for (K), dest, X.recv_counts_for (K), st, sticky); }

inline void allreduce_dev (nkp_solver *s, double *dev, int count, int op)
{
   if (!s->dist.on) return;
   s->shared->allreduce_calls++;
   if (s->dist.ops.allreduce (s->dist.ops.ctx, dev, count, op, (void *) s->stream)) s->comm_failed = true;
}

// a refactor that failed after its commit point left no usable preconditioner behind: what every later solve returns
inline int refactor_broken (const nkp_solver *s) { return fail (NKP_ESINGULAR, "%s", s->shared->why.c_str ()); }

// severity of a solve's status: OK < OK_BERR < NOT_CONVERGED < BREAKDOWN
inline int sev_of (int c) { return c == NKP_OK ? 0 : c == NKP_OK_BERR ? 1 : c == NKP_NOT_CONVERGED ? 2 : 3; }

#define NKP_BERR_ROUNDING_LEVEL 1.0e-14     // 45 eps

// ---- defined in solver.hip -------------------------------------------------------------------------------------------------
NKP_PRIVATE void solver_free (nkp_solver *s);
NKP_PRIVATE void msg (const nkp_solver *s, int lvl, const char *fmt, ...);
// ---- defined in create.hip -------------------------------------------------------------------------------------------------
// the SpMV matrix (device copy; columns may address halo slots >= n) and the matrix the preconditioner
// is built from (host only) are the same arrays except in the distributed flavour
struct SpmvMatrixHost {
   int64_t nnz, ncols;
   const int32_t *rowptr, *colind;
   const double *val;
};
// the matrix the multilevel hierarchy is built from when it is not the solver's own n x n block (distributed flavour
// with overlap: own rows followed by the overlap rows, columns renumbered accordingly)
struct PrecondMatrixHost {
   int64_t n, nblk;
   const int32_t *rowptr, *colind;
   const double *val;
   const int32_t *blk_start, *col_i, *col_j, *col_t;
};
// nkp_create (spmv_mat and pm NULL) and the rank-local part of nkp_create_dist
NKP_PRIVATE int create_impl (nkp_solver **out, const nkp_options *opt_in, int64_t n, int64_t nnz,
                             const int32_t *rowptr, const int32_t *colind, const double *val,
                             const int32_t *blk_start, int64_t nblk, int coupled_tracer_cnt, const SpmvMatrixHost *spmv_mat,
                             const PrecondMatrixHost *pm = nullptr);
// A second set of work vectors (Krylov basis, level vectors, scalars) and a second stream on the SAME device-resident
// matrix, factors and hierarchy: several right-hand sides can then be solved concurrently from different host threads,
// one clone per thread.  Single-GPU solvers only.
//
// member: the work vectors of one more system of a batched solve.  A member of a row-distributed solver shares its parent's
// matrix, hierarchy, stream, plan and exchange buffers (all of its work is ordered on that one stream) and is only ever driven
// from inside the parent's collective calls, so it adds no collective of its own.
NKP_PRIVATE int clone_impl (nkp_solver *src, nkp_solver **out, bool member);
// developer switch ml_drop_intertracer: the matrix without the couplings between its tracer_cnt tracers, i.e. exactly what a
// tracer-per-rank partition builds its rank-local hierarchies from
NKP_PRIVATE void drop_intertracer (int64_t n, int tracer_cnt, const int32_t *rowptr, const int32_t *colind, const double *val,
                                   std::vector<int32_t> &f_rowptr, std::vector<int32_t> &f_colind, std::vector<double> &f_val);
// ---- defined in krylov.hip -------------------------------------------------------------------------------------------------
// z = M r: one application of the preconditioner (one cycle)
NKP_PRIVATE void apply_precond_once (nkp_solver *s, const double *rin, double *zout);
// z = M r, optionally followed by defect-correction steps against the true operator: z += M (r - A z)
// (NKP_PRECOND_STEPS, default 1; still a fixed linear operator, so FGMRES and BiCGStab are both fine with it)
NKP_PRIVATE void apply_precond (nkp_solver *s, const double *rin, double *zout);
// y = A x (0), y = b - A x (1), y = |A||x| + |b| (2); in the distributed flavour the rows other
// ranks own are fetched first (pack -> alltoallv -> extended input vector)
NKP_PRIVATE void spmv_op (nkp_solver *s, const double *x, double *y, const double *b, int mode);
// one Arnoldi step on the device in two halves: (1) z_j = M^-1 v_j, w = A z_j; (2) orthogonalise w against V[0..j],
// v_{j+1} = w / ||w||, which leaves the Hessenberg column h[0..j+1] in s->h_dev().  The batched driver replaces (1) by
// ONE application of the cycle and of A to K interleaved vectors and runs (2) per system.
NKP_PRIVATE void arnoldi_apply (nkp_solver *s, int j);
NKP_PRIVATE void arnoldi_orthogonalise (nkp_solver *s, int j);
// one step as fgmres runs it, up to the Hessenberg column in s->hpin (tuning step_glue bit 8: krylov.hip); ev: the event
// of StepEvent, or NULL.  Whoever drives it clears s->ml.entered when no further step follows.
NKP_PRIVATE int arnoldi_hand_over (nkp_solver *s, int j, hipEvent_t ev);
// the event a run of such steps waits on (made only where tuning step_glue bit 8 can use it), destroyed with the object
struct NKP_PRIVATE StepEvent {
   hipEvent_t ev = nullptr;
   int make (const nkp_solver *s);
   ~StepEvent ();
};
// The FGMRES state machine (FgmresState and its host arithmetic: krylov_host.h) around the device work of one system.
// ||b||, the trivial case b = 0; returns a negative code on failure
NKP_PRIVATE int fg_begin (nkp_solver *s, FgmresState &F);
// true residual, verdict, start vector of the next restart cycle.  After it either F.finished, or v_0 is in place (F.j = 0).
NKP_PRIVATE int fg_restart (nkp_solver *s, FgmresState &F);
// column j of the Hessenberg matrix is in s->hpin[0 .. j+1] (copied and synchronised by the caller): Givens rotations, the
// residual estimate.  Returns true when this system's restart cycle ends here (estimate met, breakdown, column budget).
NKP_PRIVATE bool fg_post_step (nkp_solver *s, FgmresState &F);
// y = H^-1 g (upper triangular, size F.j), x += Z y; after a breakdown the true residual of what we have decides
NKP_PRIVATE int fg_end_cycle (nkp_solver *s, FgmresState &F);
// nkp_last_error of a right-hand side that fg_begin / bicgstab did not solve (s->rhs_class RHS_NONFINITE or RHS_OUT_OF_RANGE);
// `what` names it ("nkp_solve: the right-hand side").  Returns NKP_BREAKDOWN.
NKP_PRIVATE int rhs_refused (int verdict, const char *what);
// componentwise backward error of s->x for s->b, like SuperLU's berr
NKP_PRIVATE int backward_error (nkp_solver *s, double *berr);
inline SolveControls controls_of (const nkp_solver *s) { return { s->opt.max_iters, s->opt.rtol, s->opt.atol }; }
inline void controls_into (nkp_solver *s, const SolveControls &c) { s->opt.max_iters = c.max_iters; s->opt.rtol = c.rtol; s->opt.atol = c.atol; }

// ---- defined in batch_solve.hip --------------------------------------------------------------------------------------------
// per-column controls and guess flags of nkp_solve_batch_device_ex: nrhs entries each or NULL; an entry "leave as it is"
// (negative rtol / atol, max_iters 0) is the solver's own value.  The entries have been validated by the caller
struct ColumnControls {
   const double *rtol, *atol;
   const int *max_iters, *use_guess;
};
// nkp_solve_batch_device (cc NULL) and nkp_solve_batch_device_ex after their argument checks: groups, fallbacks, verdicts
NKP_PRIVATE int solve_batch_columns (nkp_solver *s, int nrhs, const void *d_B, void *d_X, int64_t ldb, const ColumnControls *cc, double *berr, int *iters, double *relres);
// what keeps a solver's right-hand sides out of the lockstep driver (NULL: nothing), and the one line a batched call that
// falls back leaves at -D1
NKP_PRIVATE const char *batch_unsupported (const nkp_solver *s);
NKP_PRIVATE void note_fallback (const nkp_solver *s, const char *who, const char *why, int nrhs);
// the K-wide buffers of a row-distributed solver (bxe, gmsg and those of its exchanges), all or nothing: the part of the
// batched solve's preparation that nkp_value_gradient shares
NKP_PRIVATE int batch_prepare_exchange (nkp_solver *s, int K);
// Row-distributed solvers: one number from every rank.  A rank whose own step failed (local_rc) contributes -1, keeps its message
// and gets its code back; a failed allgather is NKP_ECOMM everywhere.  failed_rank: the first rank that contributed -1, or -1.
// dist_agree: every rank learns whether any rank's step failed, and all leave together, the other ranks with NKP_ECOMM naming it
NKP_PRIVATE int dist_allgather (nkp_solver *s, int local_rc, int64_t mine, std::vector<int64_t> &all, const char *who, const char *where);
inline int failed_rank (const std::vector<int64_t> &all) { for (size_t p = 0; p < all.size (); p++) if (all[p] < 0) return (int) p; return -1; }
NKP_PRIVATE int dist_agree (nkp_solver *s, int local_rc, const char *who, const char *where);
// ---- defined in row_exchange.hip -------------------------------------------------------------------------------------------
// exchange_install: counts and device memory of an exchange -- send_idx (`rows` uploaded unless NULL), recv_idx where it unpacks,
// send / recv for cap_send / cap_recv rows, K wide later bsend for as many and brecv for wide_recv rows (-1: no such buffer).
// push_wide: the K-wide buffers of an exchange in force into a buffer_set
NKP_PRIVATE bool exchange_install (nkp_solver *s, RowExchange &X, const int32_t *rows, const std::vector<int> &give, const std::vector<int> &need,
                                   bool unpacks, int64_t cap_send, int64_t cap_recv, int64_t wide_recv);
NKP_PRIVATE void exchange_release (RowExchange &X);
inline void push_wide (RowExchange &X, bool in_force, std::vector<std::pair<double **, size_t>> &set)
{
   if (in_force && X.wide_send >= 0) set.push_back ({ &X.bsend, (size_t) X.wide_send });
   if (in_force && X.wide_recv >= 0) set.push_back ({ &X.brecv, (size_t) X.wide_recv });
}
inline double *halo_rows_of (nkp_solver *s, int K) { return K == 1 ? s->dist.xe + s->n : s->dist.bxe + s->n * K; }
// The input of a product with A in xe (K = 1) / bxe: own rows into place, the rows the peers need packed, the halo exchanged behind
// them on `comm` (dist.comm_stream: after the packing, ev_halo marks its end).  x: one vector, or the own rows of bxe; xp: K vectors
NKP_PRIVATE int halo_fetch (nkp_solver *s, int K, const double *x, const double *const *xp, hipStream_t comm, bool sticky = true);
// The product with the exchange under way (dist.overlap): the interior row blocks (no off-rank column) are multiplied while the
// halo travels on its own stream, the boundary rows once it has landed -- every row is still summed in stored order, so the
// result is the bit pattern of the serial version.  rows (rb0, rb1) multiplies row blocks [rb0, rb1)
template <class Rows> inline void halo_product_overlapped (nkp_solver *s, int K, const double *x, Rows rows)
{
   auto &D = s->dist;
   halo_fetch (s, K, x, nullptr, D.comm_stream);
   rows (D.seg_rb[1], D.seg_rb[2]);
   (void) hipStreamWaitEvent (s->stream, D.ev_halo, 0);
   rows (D.seg_rb[0], D.seg_rb[1]);
   rows (D.seg_rb[2], D.seg_rb[3]);
}
// ---- defined in smooth_exchange.hip ----------------------------------------------------------------------------------------
// the fine-level exchange of a row-distributed solver (tuning dist_smooth_exchange).  smooth_install: the plan's lists, counts
// and one-vector buffers into s->dist.x_smooth (nkp_create_dist; false = out of device memory).  smooth_build_lists: the device index
// lists in level-0 positions from the hierarchy s->ml holds now -- after ml_setup and after every rebuild (0, -2 no memory, -3 HIP
// failure or a hierarchy that is not the plan's).  smooth_hook_of: what the cycle applications of s take (NULL when not in force)
NKP_PRIVATE bool smooth_install (nkp_solver *s, const DistPlan &D);
NKP_PRIVATE int smooth_build_lists (nkp_solver *s);
NKP_PRIVATE const MlSmoothHook *smooth_hook_of (nkp_solver *s);
// one thread per row: out[i] = x[idx[i]] / x[idx[i]] = in[i], K interleaved vectors (K = 1, 2, 4, 8)
NKP_PRIVATE void launch_smooth_pack (int K, const int *idx, const double *x, double *out, int64_t nrows, hipStream_t st);
NKP_PRIVATE void launch_smooth_unpack (int K, const int *idx, const double *in, double *x, int64_t nrows, hipStream_t st);
// ---- defined in valgrad_api.hip --------------------------------------------------------------------------------------------
// (the *_release and *_time_prepare functions of the next three units rest on release_buffers and time_width_ok, operand_call.h;
// the *_time_* pairs are the rows of nkp_time_kernel's table, inspect.hip)
NKP_PRIVATE void valgrad_release (nkp_solver *s);
// nkp_time_kernel, which = 5: scratch operands for the gradient kernel at interleave width K (1, 2, 4, 8), then one launch
NKP_PRIVATE int valgrad_time_prepare (nkp_solver *s, int K, int which);
NKP_PRIVATE void valgrad_time_launch (nkp_solver *s, int K);
// The operand x of a K-wide kernel on the pattern (xp = the vectors, own rows; pointers beyond them NULL): single-GPU the vectors
// themselves (K = 1) or their K-interleaved copy in `il` (n * K doubles); row-distributed [own | halo] rows in dist.xe (K = 1) or
// dist.bxe (K >= 2, batch_prepare_exchange done), the halo rows of all vectors fetched in ONE alltoallv (halo_fetch), which is
// always made and counted.  *x_in = what the kernel reads.  NKP_ECOMM when the exchange failed (the stream is then still to be synchronised).
NKP_PRIVATE int fetch_x_operand (nkp_solver *s, int K, const double *const *xp, double *il, const double **x_in, const char *who);
// ---- defined in valprod_api.hip (product_stage, shared with valprod_trans_dist.hip: operand_call.h) ------------------------
NKP_PRIVATE void valprod_release (nkp_solver *s);
// nkp_time_kernel, which = 6: scratch operands for the product kernel at interleave width K (1, 2, 4, 8), then one launch;
// which = 7: the composition of SpMV kernels it replaces (product into a temporary, de-interleave, update pass)
NKP_PRIVATE int valprod_time_prepare (nkp_solver *s, int K, int which);
NKP_PRIVATE void valprod_time_launch (nkp_solver *s, int K);
NKP_PRIVATE void valprod_time_composition (nkp_solver *s, int K);
// which = 9: the same kernel on the transposed index with gathered values (nkp_values_product_trans); which = 10: the composition
// it replaces -- the values gathered into a temporary of nnz doubles, then the product kernel on the transposed pattern
NKP_PRIVATE void valprod_time_launch_trans (nkp_solver *s, int K);
NKP_PRIVATE void valprod_time_composition_trans (nkp_solver *s, int K);
// ---- defined in residual_api.hip -------------------------------------------------------------------------------------------
NKP_PRIVATE void residual_release (nkp_solver *s);
// nkp_time_kernel, which = 11: scratch operands for the residual kernel at interleave width K (1, 2, 4, 8), then one launch (R not
// written); which = 12: the composition it replaces, per column the mode-1 and mode-2 SpMV launches, launch_berr and two launch_dot
NKP_PRIVATE int residual_time_prepare (nkp_solver *s, int K, int which);
NKP_PRIVATE void residual_time_launch (nkp_solver *s, int K);
NKP_PRIVATE void residual_time_composition (nkp_solver *s, int K);
// ---- defined in transpose.hip ----------------------------------------------------------------------------------------------
// the owner frees its transposed solver and the value map; a transposed solver that is destroyed leaves its owner
NKP_PRIVATE void trans_release (nkp_solver *s);
NKP_PRIVATE void trans_detach (nkp_solver *t);
// the transposed solver and its batch members follow the owner's stream
NKP_PRIVATE void trans_set_stream (nkp_solver *s);
NKP_PRIVATE int64_t trans_device_bytes (const nkp_solver *s);
// valT = A.val[trans_src] on the owner's stream, into a buffer the owner keeps
NKP_PRIVATE int trans_gather_values (nkp_solver *s, const double **d_valT);
// out[p] = val[src[p]], p < nnz
NKP_PRIVATE void launch_tr_gather (const double *val, const int *src, int64_t nnz, double *out, hipStream_t st);
// ---- defined in transpose_dist.hip -----------------------------------------------------------------------------------------
// collective: the values of A^T's row block from the owner's new values (gather, one alltoallv, placement), then the refactor
// `refactor` (nkp_refactor_dist_device's sequence) on the transposed solver; non-zero on every rank when it could not follow
NKP_PRIVATE int trans_dist_follow (nkp_solver *s, int flags, const char *who, int (*refactor) (nkp_solver *t, const void *d_val, int flags, const char *who));
