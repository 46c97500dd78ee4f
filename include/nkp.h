/* nkp.h -- C ABI of the MI355X-native sparse solve path (libnkp_hip.so).
 *
 * This is the drop-in boundary for the one thing the reference delegates to SuperLU_DIST:
 * "factor A once, then solve A x = b for each tracer right-hand side".  Every entry point
 * names the reference call site it replaces (paths relative to /root/reference):
 *
 *   nkp_create        <- dCreate_CompCol_Matrix_dist + set_default_options_dist +
 *                        ScalePermstructInit + LUstructInit + pdgssvx_ABglobal(nrhs=0)
 *                        src/solve_ABglobal.c:327-353  (factor-only call :353)
 *   nkp_create_dist   <- dCreate_CompRowLoc_Matrix_dist + pdgssvx(nrhs=0)
 *                        src/solve_ABdist.c:482-483, 518 (row block m_loc/fst_row :141-144)
 *   nkp_solve         <- pdgssvx_ABglobal(options.Fact=FACTORED, nrhs=1): B in, X out in the
 *                        same buffer, berr out, info as return code
 *                        src/solve_ABglobal.c:363, 393-395;  src/solve_ABdist.c:571
 *   nkp_destroy       <- Destroy_CompCol_Matrix_dist, Destroy_LU, ScalePermstructFree,
 *                        LUstructFree, superlu_gridexit   src/solve_ABglobal.c:412-424
 *   nkp_spmv          <- pdgsmv_AXglobal, the SpMV inside SuperLU's refinement loop
 *                        src/SuperLU_brief_tree.txt:21-22
 *   nkp_precond_apply <- pdgstrs_Bglobal (the triangular-solve phase)
 *                        src/SuperLU_brief_tree.txt:17
 *
 * Conventions (mirroring the reference): 0 = success, non-zero = failure; diagnostics go to
 * stderr prefixed "(rank)"; all indices 0-based; CSR, as the reference writes it with sorted,
 * duplicate-free rows (src/matrix.c:3826-3832; what else a row may hold: nkp_create).  Unlike SuperLU (which takes ownership of the arrays and frees
 * them in Destroy_*_Matrix_dist) nkp_create COPIES the caller's arrays to the device and
 * never frees or keeps host pointers.
 *
 * Plain C types only; no torch / HIP types in any signature.  Device pointers are passed
 * as void* and must belong to the device the solver was created on.
 */
#ifndef NKP_H
#define NKP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NKP_VERSION 1

typedef struct nkp_solver nkp_solver;

enum nkp_precond {
   NKP_PRECOND_NONE = 0,
   NKP_PRECOND_COLUMN_JACOBI = 1,   /* exact solve of every water-column block (= column-ILU(0):
                                       zero fill outside the column's band)                   */
   NKP_PRECOND_MULTILEVEL = 3       /* column blocks as smoother inside an aggregation hierarchy */
};

enum nkp_krylov { NKP_KRYLOV_FGMRES = 0, NKP_KRYLOV_BICGSTAB = 1 };

/* return codes of nkp_solve (SuperLU's `info` analogue) */
enum {
   NKP_OK = 0,
   NKP_NOT_CONVERGED = 1,    /* max_iters reached; x holds the best iterate, NOT written by the CLIs */
   NKP_BREAKDOWN = 2,        /* the iteration broke down, or the system was not solved at all: a right-hand side or an initial
                                guess the solve refuses (see nkp_solve); x is NOT written by the CLIs */
   NKP_OK_BERR = 3,          /* ||b-Ax||/||b|| stopped above rtol at the attainable f64 accuracy, but the componentwise
                                backward error is <= max (1e-14, rtol/100); x is written; callers decide (the CLIs accept it
                                only with NKP_ACCEPT_BERR=1 in the environment) */
   NKP_EINVAL = -1,
   NKP_ENOMEM = -2,
   NKP_EDEVICE = -3,         /* HIP runtime failure / no gfx950 device */
   NKP_ESINGULAR = -4,       /* zero pivot inside a water-column block */
   NKP_ECOMM = -5
};

/* Tuning knobs of the solve path (all optional).  The defaults are the measured best (DESIGN.md sections 2, 4, 11); everything
 * else exists for A/B runs and tests.  A solver reads them ONCE, in nkp_create: from nkp_options.tuning when the caller sets
 * it, else from nkp_default_tuning, which starts from the defaults and applies the NKP_* environment variables named on the
 * right (how the reference-shaped executables, which have no room for options, are steered).  They are per solver: nothing in
 * a solve, a cycle or a kernel launch looks at the environment. */
typedef struct nkp_tuning {
   int struct_size;          /* = sizeof(nkp_tuning), ABI guard */
   /* ---- hierarchy construction */
   int ml_split;             /* NKP_ML_SPLIT (1): connectivity-aware coarse cells inside the geometric groups */
   int ml_pocket;            /* NKP_ML_POCKET (4): same-depth connected sets of at most that many cells become one coarse cell */
   int ml_big_from;          /* NKP_ML_BIG_FROM (-3 = automatic): 4 x 4 groups from that level on, -1 = never */
   int ml_coarsest_rows;     /* NKP_ML_COARSEST_ROWS (8000): stop coarsening at that many rows (a dense level costs its bytes, an iterated one ~200 us of launch latencies) */
   int ml_dense_max;         /* NKP_ML_DENSE_MAX (8192): largest last level solved with a dense inverse */
   double ml_theta;          /* NKP_ML_THETA (0): edge threshold of the connectivity test */
   double ml_tau;            /* NKP_ML_TAU (0.01): leaf-stub threshold */
   int64_t ml_device_min;    /* NKP_ML_DEVICE_MIN (100000): levels with at least that many rows are built by the setup kernels,
                                smaller ones on the host (same hierarchy either way); < 0 = host only */
   /* ---- cycle */
   int ml_smooth_coarse;     /* NKP_ML_SMOOTH_COARSE (0 = like the fine levels): sweeps on levels >= ml_coarse_from */
   int ml_coarse_from;       /* NKP_ML_COARSE_FROM (2) */
   int ml_gamma_from, ml_gamma_to;   /* NKP_ML_GAMMA_FROM / _TO (0, 0): levels [from, to) visit the coarse level twice */
   int ml_f32;               /* NKP_ML_F32 (1): level operators and column factors stored in f32 (arithmetic in f64) */
   int ml_host_inverse;      /* NKP_ML_HOST_INVERSE (0): dense inverse of the last level on the host */
   int ml_fused;             /* NKP_ML_FUSED (0): one launch per Gauss-Seidel half sweep */
   int ml_fused_max_cols;    /* NKP_ML_FUSED_MAX_COLS (0 = all): ... only on levels with at most that many columns */
   int ml_wave_fused;        /* NKP_ML_WAVE_FUSED (1): levels solved one column per wave run each half sweep as ONE launch;
                                0 = never, N > 1 = only levels with at most N columns */
   int ml_coarsest_sweeps;   /* NKP_ML_COARSEST_SWEEPS (30): sweeps on a last level too large for a dense inverse */
   int64_t ml_tail_rows;     /* NKP_ML_TAIL_ROWS (0): the last levels with at most that many rows in one launch */
   double ml_omega;          /* NKP_ML_OMEGA (1.1): weight of the coarse-grid correction */
   /* ---- water-column solves: which kernel serves which level */
   int col_ldsres;           /* NKP_COL_LDSRES (2) */
   int col_stream;           /* NKP_COLSTREAM (1) */
   int col_stream_min;       /* NKP_COLSTREAM_MIN (-1 = per-kernel defaults) */
   int col_stream_gw;        /* NKP_COLSTREAM_GW (32) */
   int col_wave_max;         /* NKP_COLWAVE_MAX (8192): levels with at most that many columns solve one column per wave */
   int col_w3;               /* NKP_COL_W3 (1) */
   int col_group;            /* NKP_COLGROUP (8) */
   int col_pipe_min;         /* NKP_COLPIPE_MIN (0 = off) */
   int col_ldsres_early;     /* NKP_LDSRES_EARLY (0) */
   int col_ldsres_packed;    /* NKP_COL_PACKED (1): LDS-resident column kernel with factors packed four steps to a 16-byte load */
   /* ---- CSR SpMV launch shape */
   int spmv_variant;         /* NKP_SPMV_VARIANT (4): 0 .. 4 load flavours of the stream kernel (4 pipelined from spmv_pipe_min row blocks on), 9 rows kernel; the environment's values outside 0 .. 9 count as 4 */
   int spmv_compress;        /* NKP_SPMV_COMPRESS (0): 2-byte column codes */
   int spmv_pipe_min;        /* NKP_SPMV_PIPE_MIN (1024): fewest row blocks for the pipelined kernel */
   int spmv_run;             /* NKP_SPMV_RUN (1): row blocks one workgroup walks */
   int spmv_wgs;             /* NKP_SPMV_WGS (256): workgroups per CU at most */
   /* ---- Krylov / distributed flavour / setup */
   int rhs_batch;            /* NKP_RHS_BATCH (1): several right-hand sides of one call share the sweeps over the matrix and the
                                hierarchy (nkp_solve_batch_device; same bits per column, also under equil and precond_steps >= 2;
                                its comment lists what still goes one at a time); 0 = one at a time, 1 or 4 = groups of up to
                                four, 2 = pairs, 8 = groups of up to eight (measured at 1 degree: no better per solve than four -- with
                                four vectors interleaved the vectors, not the matrix, are most of every kernel's bytes) */
   int precond_steps;        /* NKP_PRECOND_STEPS (0 = leave nkp_options.precond_steps) */
   int equil;                /* NKP_EQUIL (-1 = leave nkp_options.equil) */
   int dist_overlap;         /* NKP_DIST_OVERLAP (1): halo exchange behind the interior rows */
   int dist_ras;             /* NKP_DIST_RAS (1): one ring of the neighbours' columns in the rank's hierarchy */
   int force_dist;           /* NKP_FORCE_DIST (0): distributed code path with one rank */
   int setup_threads;        /* NKP_SETUP_THREADS (0 = automatic): host threads of the setup loops */
   int plan_times;           /* NKP_ML_PLAN_TIMES (0): print the split of the host-side aggregation */
   int ml_drop_intertracer;  /* NKP_ML_DROP_INTERTRACER (0): developer switch, hierarchy without inter-tracer couplings */
   int dist_one_reduce;      /* NKP_DIST_ONE_REDUCE (0): distributed Arnoldi step with ONE allreduce -- the norm of the orthogonalised
                                vector comes from the reduced multi-dot message (w.w - sum h^2) instead of a second allreduce.
                                Off by default: the identity assumes an orthonormal basis, which one Gram-Schmidt pass keeps only
                                to 1e-6 or so, and the solve pays for it (2 ranks, 40x46x20: 48 iterations against 45) -- more than
                                the 20-30 us allreduce it saves per 3 ms step */
   int ml_huge_from;         /* NKP_ML_HUGE_FROM (-1 = never): 8 x 8 groups from that level on */
   int col_ldsres_min;       /* NKP_COL_LDSRES_MIN (0 = automatic): fewest columns of a level served by the LDS-resident column kernels */
   int col_sort_groups;      /* NKP_COL_SORT_GROUPS (1): packed column layout groups a colour's columns by length (less zero padding) */
   int batch_spmv_rows;      /* NKP_BATCH_SPMV_ROWS (1): batched SpMV stages the (value, column) stream in LDS and lets each row's lane gather
                                its own K-wide rows of x; 0 = products parked in LDS, K / 2 passes */
   int dist_ras_rings;       /* NKP_DIST_RAS_RINGS (1): depth of the overlap that dist_ras gives each rank's hierarchy, in rings of other
                                ranks' water columns (ring k + 1 = the lateral columns that rows of ring k couple to); 2 .. 4 ask for that
                                many, 0 = the default, anything else is NKP_EINVAL.  The ranks take the smallest depth any of them asks for.
                                With two or more rings the overlap residual travels in an exchange of its own (still one per preconditioner
                                application) instead of riding on the SpMV halo.  No effect without dist_ras, grid positions or a lateral
                                cut (a tracer partition has no overlap) */
   int ml_diag;              /* NKP_ML_DIAG (32): level operators also stored as per-column diagonals, which the residual rows of the
                                two-kernel half sweeps, the wave-fused half sweeps of a level whose columns have at most 64 rows and
                                the residual before the restriction then read instead of CSR (no per-entry column index; same bits).
                                N > 0 = a level gets them if no water column needs more than N diagonals and the padding stays
                                within 1.5 x its entries, else it stays on CSR; 0 = off */
   int spmv_diag;            /* NKP_SPMV_DIAG (32): the solver's own matrix A also stored as per-column diagonals (f64 values), which
                                y = A x and y = b - A x of nkp_spmv, the Krylov drivers and the chained cycles then read instead of
                                CSR.  Same meaning as ml_diag: N > 0 = A gets them if no water column of the caller's blk_start
                                needs more than N diagonals and the padding stays within 1.5 x its entries; 0 = off.  CSR is kept
                                -- silently -- when no blk_start was given, on a row-distributed solver (NKP_FORCE_DIST included:
                                the halo columns live behind n) and on a transposed handle, and by everything else that reads A
                                (|A||x| + |b|, the K-vector products, nkp_values_product, nkp_value_gradient, the setup).  Every
                                row is summed from +0.0 in stored order, so the bits are those of the CSR kernels for finite x; the
                                one difference: a padded slot holds +0.0, and +0.0 times a non-finite x is NaN where CSR would not
                                touch that x (the level operators under ml_diag behave the same) */
   int ml_lane_fused;        /* NKP_ML_LANE_FUSED (50000): levels of the cycle on the packed lane-per-column layout with at most that many
                                water columns, columns of at most 64 rows, half bandwidth <= 2 and their operator on diagonals (ml_diag)
                                run every Gauss-Seidel half sweep as ONE launch (gs_lanes_diag_kernel: residual rows per wave, band
                                solves per lane) instead of residual rows + column solves; same bits.  0 = off */
   int dist_smooth_exchange; /* NKP_DIST_SMOOTH_EXCHANGE (0): 1 = on a row-distributed multilevel solver whose hierarchy has an overlap
                                (dist_ras; see dist_ras_rings) every Gauss-Seidel half sweep on level 0 of the cycle is followed by an
                                exchange that overwrites x on that colour's overlap rows, over all rings, with their owners' values: the
                                own rows then see the global two-colour water-column Gauss-Seidel instead of one cut at the rank's
                                edge ("fine-level exchange").  The exchange after the cycle's last half sweep
                                is left out (nothing reads those rows), so one cycle makes 2 (nu_pre + nu_post) - 1 more alltoallv
                                calls of device doubles -- 11 with V(3, 3) -- each of rows x 8 bytes per neighbour (x K for a batched
                                group, which makes the exchanges of one system); they run in line on the solver's stream, after the
                                overlap residual's exchange of the same application, in the same order on every rank whatever its
                                lists hold, and are counted in "dist_alltoallv_calls".  Any value other than 0 or 1 is NKP_EINVAL,
                                refused by every rank together like a dist_ras_rings out of range.  The ranks take the smallest value any of
                                them asks for; the agreement rides on the message that settles the overlap depth, so nkp_create_dist
                                has no collective more than without it.  No effect without dist_ras, grid positions or a lateral
                                cut (a tracer partition has no overlap), or on one rank; and none unless level 0 of EVERY rank's
                                hierarchy runs the same half sweeps (a rank whose [own | overlap] block is small enough to be one
                                dense level, ml_coarsest_rows, has none: its sweep count rides on the last agreement of
                                nkp_create_dist, and the ranks then leave the exchange out together).  nkp_get_int
                                "dist_smooth_exchange" tells what is in force.  The hierarchy of a refactor that rebuilds must keep a
                                smoothed level 0, else the refactor fails at its commit agreement */
   int step_glue;            /* NKP_STEP_GLUE (12): bit mask of what a Krylov step leaves out between its large kernels; every stored double
                                keeps its bits, 0 = every launch of its own.  4 = the restriction of the single-vector cycle also zeroes
                                the coarse level's x (every level but a dense last one) and requests a coarse row's fine values
                                together.  8 = FGMRES, not row-distributed, no row equilibration, one cycle per iteration: the kernel that
                                completes the Hessenberg column adds up ||w||^2 itself and stores the column to pinned host memory as
                                well, and the host waits on an event behind that kernel instead of copying and synchronising the
                                stream; with an f64 basis and the multilevel preconditioner one kernel then writes v = w / ||w|| to
                                the basis and to level 0's right-hand side and zeroes level 0's x (instead of scale, gather, fill), and
                                it and the first column solves of level 0 are enqueued before the wait and run while the host decides.
                                Not for the last slot of a restart cycle.  Bits 1 and 2 are not used */
} nkp_tuning;

/* defaults, then the NKP_* environment overrides listed above */
int nkp_default_tuning (nkp_tuning *t);

typedef struct nkp_options {
   int struct_size;      /* = sizeof(nkp_options), ABI guard                                  */
   int precond;          /* enum nkp_precond                                                  */
   int krylov;           /* enum nkp_krylov                                                   */
   int restart;          /* FGMRES restart length m                                           */
   int max_iters;        /* total Krylov iterations allowed per right-hand side               */
   double rtol;          /* stop when ||b - A x||_2 <= rtol * ||b||_2 (true residual)         */
   double atol;          /* ... or <= atol   (these three: nkp_set_solve_controls later on)   */
   int device;           /* HIP device ordinal; -1 = leave the current device                 */
   int verbose;          /* the reference's dbg_lvl: 0 silent, 1 progress, 2 per-iteration    */
   int rank;             /* printed as the "(rank)" message prefix (reference `iam`)          */
   int reorth;           /* 0 = one classical Gram-Schmidt pass (default), 1 = two passes     */
   int ml_levels;        /* multilevel: max levels (0 = automatic)                            */
   int ml_smooth;        /* multilevel: smoothing sweeps per level per half-cycle             */
   int basis_f32;        /* 1: store the Krylov basis V in f32 for the Gram-Schmidt passes (the solution update uses
                            the f64 Z vectors, the true residual is recomputed in f64 at every restart).  Default 0:
                            with a single Gram-Schmidt pass the f32 basis can double the iteration count. */
   int precond_steps;    /* preconditioner cycles per Krylov iteration, chained by defect correction against A:
                            z = M r; z += M (r - A z); ...  0 = automatic (= 1 since round 2) */
   int equil;            /* row equilibration (SuperLU's Equil=YES, reference src/solve_ABglobal.c:332): FGMRES minimises
                            ||R (b - A x)||_2 with R = diag (1 / max_j |a_ij|) instead of ||b - A x||_2; the stopping test
                            stays on the unscaled residual.  0 = automatic (off unless NKP_EQUIL=1), 1 = on, -1 = off.
                            Column scaling has no effect on a right-preconditioned iteration and is not applied. */
   int reserved[4];
   /* multilevel, optional: grid position (i, j) of every water-column block, nblk entries each
    * (tracer_state_ind_to_i/_j at the block's first row, reference src/matrix.c:322-329).  With
    * them columns are aggregated 2 x 2 in (i, j) and coloured (i + j) % 2; without them
    * (NULL) the setup falls back to pairwise matching on the column graph.  Host pointers, read
    * during nkp_create only. */
   const int32_t *col_i;
   const int32_t *col_j;
   /* optional: tracer of every water-column block (nblk entries).  NULL = tracer-major rows (reference
    * src/matrix.c:778-784): block c belongs to tracer c / (nblk / coupled_tracer_cnt).  Needed when the rows were
    * reordered cell-major (nkp_cell_major_order below).  Columns of different tracers are never aggregated together. */
   const int32_t *col_t;
   /* optional: tuning knobs (NULL = nkp_default_tuning: defaults + NKP_* environment).  Read during nkp_create only. */
   const nkp_tuning *tuning;
} nkp_options;

int nkp_default_options (nkp_options *opt);

/* Number of visible HIP devices (0 when there is no GPU); never fails. */
int nkp_device_count (void);

/* Setup ("factor") -- host CSR in, device-resident solver out.
 *   blk_start[nblk+1]: row offsets of the water-column blocks (contiguous, ascending,
 *   blk_start[0]=0, blk_start[nblk]=n).  Rows of one block are the levels k=0..KMT-1 of one
 *   (tracer, column) (src/matrix.c:239-251, 778-784).  NULL => every row its own block
 *   (point Jacobi).
 *
 * What the CSR arrays may hold.  A IS THE SUM OF ITS STORED ENTRIES: every product, factor and derivative below is
 * of that sum, whatever the order of a row and however often a column is repeated in it.
 *   NKP_PRECOND_NONE, NKP_PRECOND_COLUMN_JACOBI   rows in any order; a column may be repeated in a row (the entries
 *        add up, in the products and in the factored water-column blocks alike); stored zeros are entries like any
 *        other.  NKP_PRECOND_NONE also takes rows without entries.  Only strictly ascending rows can run on the
 *        per-column diagonals of nkp_tuning.spmv_diag; A with any other row stays on CSR, with the same products.
 *   NKP_PRECOND_MULTILEVEL   strictly ascending rows only (sorted by column, no column repeated; what gen_A writes):
 *        the setup looks entries up by bisection.  Anything else is refused with NKP_EINVAL "not sorted by column".
 * Both preconditioners need a non-zero diagonal in every row, judged on the SUM of the row's diagonal entries in
 * stored order: a diagonal stored as +1, -1 is refused with NKP_ESINGULAR like a missing one, by nkp_create and by
 * nkp_refactor*.  Per-entry results (nkp_value_gradient, nkp_values_product, nkp_refactor's values) follow the stored
 * order entry by entry; the parts of a repeated entry each get the gradient of the coupling they add up to. */
int nkp_create (nkp_solver **out, const nkp_options *opt, int64_t n, int64_t nnz,
                const int32_t *rowptr, const int32_t *colind, const double *val,
                const int32_t *blk_start, int64_t nblk, int coupled_tracer_cnt);

/* Same with 64-bit row pointers (what a CDF-5 matrix file or a caller that counts entries in int64 holds).  Entry
 * offsets are stored in 32 bits on the device, so ONE GPU takes at most 2^31 - 1 entries (25 GB of values and column
 * indices); a larger system is row-partitioned with nkp_create_dist, where the limit applies to each rank's block --
 * the 0.25 degree x 4 tracer system (4.2 G entries, n = 203 M < 2^31) is representable on 4 or 8 ranks.  Returns
 * NKP_EINVAL with that explanation when rowptr[n] does not fit. */
int nkp_create64 (nkp_solver **out, const nkp_options *opt, int64_t n, const int64_t *rowptr /* n+1 */,
                  const int32_t *colind, const double *val, const int32_t *blk_start, int64_t nblk, int coupled_tracer_cnt);

/* Solve nrhs systems; b (host, column-major, leading dimension ldb >= n) is overwritten by x
 * when the return code is NKP_OK or NKP_NOT_CONVERGED.  berr[r] receives the componentwise
 * backward error max_i |b-Ax|_i / (|A||x|+|b|)_i like SuperLU's; iters/relres per rhs.
 * Any of berr/iters/relres may be NULL.
 * NKP_OK means ||b-Ax||/||b|| <= rtol (or <= atol absolute) on the true residual, nothing else.  When rounding
 * stops the residual above rtol (badly scaled rows: even a direct solve with refinement then stays above it) the solve
 * ends after a few restart cycles instead of running to max_iters and returns NKP_OK_BERR if the componentwise
 * backward error -- the accuracy measure the reference itself reports (berr, src/solve_ABglobal.c:396-398) -- is
 * <= max (1e-14, rtol / 100), else NKP_NOT_CONVERGED.
 * nrhs >= 2 right-hand sides share the sweeps and, on a row-distributed solver, the collectives of every Krylov step
 * (nkp_solve_batch_device below; there the call is collective: the same nrhs on every rank, ldb >= m_loc).
 *
 * Vectors the solve refuses.  With ||b||^2 (the f64 sum of squares) and target = max (rtol ||b||, atol):
 *    - inside the range -- ||b||^2 finite and target >= 2^-480 (3.2e-145) -- the solve iterates; there a power of two on b is
 *      the same power of two on x, bit for bit, with the same iters, relres and berr.  (The floor is derived, not measured:
 *      target^2 < 2^-960 is 62 binary orders above the smallest normal number, so a sum of squares at the target loses less
 *      than 2^-62 of itself per term to underflow.)  ||b||^2 = 0 with atol >= 2^-480 is ||b|| < atol: x = 0, NKP_OK.
 *    - outside it the entries of b are counted (a counting kernel and, row-distributed, one more allreduce; all ranks take this
 *      path together since ||b||^2 is global).  No non-finite and no non-zero entry: b = 0, x = 0 with NKP_OK, relres 0.
 *      Anything else is NOT solved: NKP_BREAKDOWN with iters 0, relres NaN, berr NaN and EVERY entry of x NaN -- on the
 *      device and in the host array of nkp_solve, which copies x back for every status >= 0 -- and nkp_last_error says
 *      that the right-hand side "holds a non-finite entry" or "is outside the range" of the solve.  It is a status, not an
 *      error code: one bad column of several does not stop the others, and the call returns the worst status of its columns.
 *      Rescale such a system (b 2^k has the solution x 2^k).
 *    - a non-finite initial guess (nkp_solve_device with use_guess), or a residual norm that overflows on the way, is
 *      NKP_BREAKDOWN with relres NaN; with the non-finite guess berr is NaN too.
 * Every driver takes the decision from one host routine (rhs_verdict, csrc/krylov_host.cpp): FGMRES, BiCGStab, the batched
 * members, and through them the transposed solver and nkp_solve_tangent.
 * berr is NaN as soon as one entry of b - A x or of |A||x| + |b| is NaN (Inf / Inf included); otherwise the rule above.  On a
 * row-distributed solver the maximum is taken across ranks by the allreduce of the transport, and what that makes of a NaN is
 * up to the transport: there only the status and x are promised.
 * Matrix values must be finite, at nkp_create and at nkp_refactor alike; they are NOT checked, and what a solve with a NaN
 * or an Inf in A returns is not specified (a status and numbers, no fault). */
int nkp_solve (nkp_solver *s, double *b_in_x_out, int nrhs, int64_t ldb,
               double *berr, int *iters, double *relres);

/* Several right-hand sides at once -- the reference's RHS loop (src/solve_ABglobal.c:370-409) with the tracers sharing every sweep
 * over the matrix and the hierarchy: d_B / d_X hold nrhs vectors of n doubles on the solver's device, vector c at offset c * ldb
 * (d_X may alias d_B).  Systems are solved in groups of up to four; each keeps its own FGMRES recurrence and stopping test, the
 * operator and preconditioner applications of a Krylov step are one pass for the group.  Column c of the result has the bits
 * nkp_solve_device gives for that right-hand side alone, iters[c] / relres[c] / berr[c] likewise; the return code is the worst of
 * the columns'.  Needs K - 1 more sets of work vectors (kept for later calls).
 * Row equilibration (nkp_options.equil) and chained preconditioner cycles (precond_steps >= 2) are batched with the rest, alone or
 * together: the two row scalings sit in the kernels that read the basis vectors and write the operator products, and every stage
 * of a chained step -- cycle, residual v - A z, cycle, z += correction, operator -- is one pass for the group.  The run-time
 * guard that drops a solve to one cycle per step is per system, as in a solve done alone; a group may hold both kinds.
 * Falls back to one at a time, with the same answers, where the batched path does not apply:
 *    - a solver made by nkp_clone,
 *    - BiCGStab,
 *    - an f32 Krylov basis (basis_f32),
 *    - row equilibration on a row-distributed solver,
 * or with nkp_tuning.rhs_batch = 0.  With verbose >= 1 such a call prints one "(rank)"-prefixed line that names the reason.
 * nkp_solve with nrhs >= 2 takes the same path.
 *
 * On a solver made by nkp_create_dist with more than one rank the call is collective for nrhs >= 2 exactly as nkp_solve is
 * for one system: every rank calls with the same nrhs and passes its own rows of every vector (ldb >= m_loc).  A group of K
 * systems then runs in lockstep on every rank with the collectives of ONE system per Krylov step: one alltoallv of K-wide
 * rows for the overlap rows of the preconditioner, one for the halo of the SpMV, and one allreduce per Gram-Schmidt pass
 * (plus one for the norms) whose message holds the K systems' dot products.  With precond_steps = s chained cycles a step has s
 * preconditioner applications and s operator applications (s - 1 residuals and the product), each with its one exchange: 2 s
 * alltoallv per step with an overlap, s without (dist_ras = 0); the allreduces do not change.  The interleave width is agreed between the ranks
 * (allgather_i64_host): all of them take the narrowest one any rank has device memory for; a rank with another failure returns
 * its code, the others NKP_ECOMM naming it (nkp_solve agrees likewise on having staged its host vectors on the device).  Bits: column c has the bits of nkp_solve_device on right-hand side c alone
 * (solution, iters, relres, berr) whenever the transport's allreduce gives an element the same bits whatever the length of the
 * message it travels in -- the file transport (fixed rank order) with any number of ranks, any transport with two ranks.  On
 * other transports (gloo or RCCL with three or more ranks) every column meets the same stopping test on the true residual;
 * bit identity is not promised there. */
int nkp_solve_batch_device (nkp_solver *s, int nrhs, const void *d_B, void *d_X, int64_t ldb, double *berr, int *iters, double *relres);

/* Same, with b and x already resident on the solver's device (x may alias b); x_inout is also
 * the initial guess when use_guess != 0. */
int nkp_solve_device (nkp_solver *s, const void *d_b, void *d_x, int use_guess,
                      double *berr, int *iters, double *relres);

/* rtol, atol and max_iters of an existing solver -- PETSc's KSPSetTolerances: an inexact Newton driver keeps ONE solver (matrix,
 * hierarchy, work vectors) and loosens or tightens the linear solves from step to step instead of creating a solver per
 * tolerance.  Restart length, Krylov method, precond_steps and equil size or shape what nkp_create builds (the basis, the chained
 * cycles' vectors, the row scales) and stay what they were created as. */
typedef struct nkp_solve_controls {
   int struct_size;   /* = sizeof(nkp_solve_controls), ABI guard */
   int max_iters;     /* > 0; 0 = leave as it is */
   double rtol;       /* finite, >= 0; negative = leave as it is */
   double atol;       /* finite, >= 0; negative = leave as it is */
} nkp_solve_controls;

/* After nkp_set_solve_controls (s, c) every solve entry on s -- nkp_solve, nkp_solve_device, nkp_solve_batch_device,
 * nkp_solve_tangent_device, nkp_solve_batch_device_ex -- behaves BIT FOR BIT like the same call on a solver created with those
 * three values in nkp_options and everything else equal: x, iters, relres, berr, the return code and the rtol printed in
 * messages.  That covers target = max (rtol ||b||, atol) as rhs_verdict sees it (so the 2^-480 floor of nkp_solve follows the
 * new target), the NKP_OK_BERR threshold max (1e-14, rtol / 100) and the stagnation logic: the drivers read the three values
 * from the handle when a solve starts and nothing is sized by them.  c == NULL puts back the values the handle began with.
 *   The controls belong to the handle.  A clone starts with its source's values of the moment of nkp_clone, a transposed
 *   handle with its owner's of the moment nkp_transpose* built it (and those are what c == NULL gives back on it); afterwards
 *   every handle has its own, nothing propagates.  nkp_refactor* keeps them, NKP_REFACTOR_REBUILD included.  The members of a
 *   batched group are internal and follow their owner at every call.  No solve may be in flight on the handle.
 *   Refused with NKP_EINVAL, nothing changed, without any HIP call: a NULL solver, a struct_size mismatch, a NaN or an Inf in
 *   rtol / atol, max_iters < 0.
 *   Row-distributed solvers: the call is COLLECTIVE and all ranks pass the same values -- ranks with different stopping tests
 *   would part in their collectives.  The ranks agree on the bit patterns of what would be in force through three
 *   allgather_i64_host calls, always all three and in this order whatever happens locally: rtol, atol, max_iters (a rank whose
 *   own check failed sends -1).  On a mismatch, or when a rank's check failed, every rank returns NKP_EINVAL naming the lowest
 *   rank that differs from rank 0 or failed, and no rank changes anything; a failed allgather is NKP_ECOMM.  A NULL solver is
 *   refused on the calling rank before any collective.  On a plain solver (one rank without force_dist) there is no
 *   collective.
 * nkp_get_solve_controls: what is in force on the handle.  out->struct_size is set BY THE CALLER (the ABI guard; checked first,
 * then the handle): NKP_EINVAL for NULL out, a mismatch -- the message gives the library's size --, a NULL solver.
 * nkp_get_int: "max_iters". */
int nkp_set_solve_controls (nkp_solver *s, const nkp_solve_controls *c);
int nkp_get_solve_controls (nkp_solver *s, nkp_solve_controls *out);

/* nkp_solve_batch_device with per-column controls and initial guesses -- a warm start on the batched path.  rtol / atol /
 * max_iters: nrhs entries each or NULL (= the solver's, as set above); an entry "leave as it is" (negative, 0) also means the
 * solver's.  use_guess: nrhs flags or NULL; where use_guess[c] != 0, column c of d_X holds x0 on entry.
 *   Column c has the bits nkp_solve_device (s, b_c, x_c, use_guess[c], ...) gives alone on a solver whose controls are column
 *   c's: solution, iters[c], relres[c], berr[c] and status -- the promise of nkp_solve_batch_device with the controls and the
 *   guess added (on a row-distributed solver under that call's condition on the transport).  The return code is the worst of
 *   the columns'.  Groups are formed exactly as there: in order, up to the width rhs_batch allows; a column with a guess and
 *   one without may share a group.  The per-column values sit in the options of the systems' work sets while the call runs and
 *   the solver's own are back when it returns, however it returns.  Controls and guesses are honoured on every path: the
 *   batched groups, the single remainder of a group, and every fallback nkp_solve_batch_device lists (a clone, BiCGStab, an
 *   f32 basis, equil on a row-distributed solver, rhs_batch = 0).
 *   A non-finite guess in column c is that column's NKP_BREAKDOWN as documented at nkp_solve (iters 0, relres NaN, berr NaN,
 *   x_c left as it was passed); the other columns are untouched.
 *   Refused with NKP_EINVAL before any device work: a NULL solver or buffer (before the handle is looked at; the message names
 *   the argument), nrhs < 0, ldb < n, a NaN or an Inf in rtol / atol, max_iters[c] < 0, d_X == d_B while any use_guess[c] != 0
 *   (the guess and the right-hand side would be the same memory).
 *   Row-distributed solvers: collective as nkp_solve_batch_device is, and the ranks must pass identical arrays.  The call
 *   checks this with ONE allgather_i64_host of a 64-bit hash (FNV-1a over nrhs and the bytes of the four arrays, NULL-ness
 *   included) before the solve's own collectives; it is always made, also by a rank that refuses its own arguments (which then
 *   returns its own message).  A mismatch is NKP_EINVAL on every rank, naming a rank, with nothing solved and no alltoallv. */
int nkp_solve_batch_device_ex (nkp_solver *s, int nrhs, const void *d_B, void *d_X, int64_t ldb,
                               const double *rtol, const double *atol, const int *max_iters, const int *use_guess,
                               double *berr, int *iters, double *relres);

/* y = A x, exposed for parity and roofline tests (host and device flavours). */
int nkp_spmv (nkp_solver *s, const double *x, double *y);
int nkp_spmv_device (nkp_solver *s, const void *d_x, void *d_y);

/* z = M^-1 r with the configured preconditioner (host buffers). */
int nkp_precond_apply (nkp_solver *s, const double *r, double *z);

/* Deterministic device reductions used by the Krylov drivers, exposed for parity tests:
 * out[j] = sum_i V[j*ld + i] * w[i], j < k   (host buffers). */
int nkp_multi_dot (nkp_solver *s, const double *V, int64_t ld, int k, const double *w, double *out);

/* Average duration (ms) of `reps` back-to-back launches of one kernel on the solver's stream,
 * measured with HIP events on that stream.  which: 0 = CSR SpMV, 1 = preconditioner apply,
 * 2 = one full FGMRES step at restart position `arg` (0 <= arg < restart) as a solve runs it, the hand-over of the Hessenberg
 * column to the host included (tuning step_glue: the wait and what is enqueued ahead of the next step); multilevel only: 3 = the
 * smoother's residual rows of one colour of the fine level, 4 = the water-column solves of that colour; 5 = the gradient kernel of
 * nkp_value_gradient alone with K = arg in {1, 2, 4, 8} pairs of vectors, on scratch vectors of the solver (single-GPU solvers
 * only, NKP_EINVAL elsewhere and for another arg; its compulsory bytes: 12 nnz + 4 (n + 1) + 16 K n); 6 = the product kernel of
 * nkp_values_product alone with K = arg in {1, 2, 4, 8} vectors, values and vectors scratch of the solver, alpha = -1 without
 * accumulation (single-GPU solvers only, NKP_EINVAL elsewhere and for another arg; its compulsory bytes: 12 nnz + 4 (n + 1) +
 * 16 K n, plus 8 K n when accumulating -- at K = 1 exactly the SpMV's); 7 = for comparison with 6, same arg: the composition
 * that kernel replaces, made of the SpMV kernels on the solver's own values -- the (batched) operator product into a temporary, its
 * de-interleave, one update pass over the K vectors (24 K n more bytes); 8 = the product y = A x on A's per-column diagonals
 * (tuning spmv_diag; NKP_EINVAL when A has none -- 0 stays the CSR kernel on the same matrix either way); 9 = the kernel of
 * nkp_values_product_trans alone, operands and arg as for 6, on the transposed index (built by this call if the solver has none;
 * its compulsory bytes: those of 6 + 4 nnz for the value map); 10 = for comparison with 9, same arg: the composition it replaces
 * -- the values gathered through the map into a temporary of nnz doubles, then the kernel of 6 on the transposed pattern (16 nnz
 * more bytes).  9 and 10: single-GPU solvers that own their pattern only (NKP_EINVAL on a row-distributed solver, a clone, a
 * transposed handle, and for another arg); 11 = the kernel of nkp_residual_batch alone (its per-column finish included) with K =
 * arg in {1, 2, 4, 8} vectors, B and X scratch of the solver, R not written (single-GPU solvers only, NKP_EINVAL elsewhere and
 * for another arg; its compulsory bytes: 12 nnz + 4 (n + 1) + 16 K n); 12 = for comparison with 11, same arg: what a caller had
 * to compose before, column by column -- the b - A x and |A||x| + |b| products of a solve's backward error, its berr pass, and
 * two dots for the norms (2 K sweeps over A). */
int nkp_time_kernel (nkp_solver *s, int which, int arg, int reps, double *avg_ms);

/* Introspection: key = "n", "nnz", "nblk", "band", "levels", "spmv_bytes" (compulsory bytes of the CSR product: 12 nnz +
 * 4 (n + 1) + 16 n), "device_bytes", "precond_steps", "equil"; "spmv_diag" (1 = the products with A run on its per-column
 * diagonals, tuning spmv_diag), "spmv_diag_bytes" (compulsory bytes of one such product: 8 per stored slot, padding included,
 * the tile and group descriptors, 16 n; 0 without diagonals);
 * column-Jacobi preconditioner, the lane layout of its column blocks: "col_stream" (1 = factors streamed), "col_ldsres" (0, 1 =
 * column resident in LDS, 2 = packed), "col_gw" (columns per group), "col_max_len" (longest column), "col_lds_bytes" (dynamic LDS);
 * "create_us" (wall time of nkp_create), "ml_setup_us" (of which: the hierarchy), "ml_levels_on_device" (levels whose operator
 * the setup kernels built; the smaller ones are built on the host), "ml_inverse_pivoted" (1 = the last level's dense inverse came
 * from the pivoted routine, because the blocked elimination met a pivot it does not trust; 0 = blocked elimination or the host routine;
 * read it on the solver that owns the hierarchy: a clone keeps the value of the moment it was cloned, also across a refactor of its owner);
 * compulsory HBM bytes of the pieces nkp_time_kernel times: "smoother_spmv_bytes", "column_solve_bytes", "cycle_bytes";
 * distributed flavour: "dist_overlap" (halo exchange hidden behind the interior rows), "dist_interior_rowblocks",
 * "dist_ras" (hierarchy overlaps the neighbouring ranks), "dist_ras_rows" (rows of other ranks in this rank's hierarchy, all rings),
 * "dist_ras_rings" (the depth the ranks agreed on, 0 without overlap), "dist_halo_rows" (rows received before every SpMV),
 * "dist_ras_recv_rows" (rows received per preconditioner application: the SpMV halo with one ring, the overlap rows with more);
 * "dist_smooth_exchange" (1 = the fine-level exchange of tuning dist_smooth_exchange is in force: a Krylov step then has, per cycle,
 * the overlap residual's alltoallv, then 2 (nu_pre + nu_post) - 1 alltoallv calls of the half sweeps, then those of the SpMV and the
 * allreduces as before), "dist_smooth_rows" (overlap rows refreshed per pair of half sweeps, = "dist_ras_rows" when in force, else 0);
 * counters, cumulative over the solver's life, per rank: "dist_alltoallv_calls", "dist_allreduce_calls" (every call of the two
 * device collectives made by solves, single or batched, and the one alltoallv of every nkp_value_gradient*; 0 on a single-GPU
 * solver), "value_gradient_calls" (successful nkp_value_gradient* calls), "value_gradient_us" (wall time of the last one),
 * "values_product_calls" (successful products: nkp_values_product* calls and the one inside every nkp_solve_tangent_device with
 * d_dval), "values_product_us" (wall time of the last one), "tangent_calls" (nkp_solve_tangent_device calls that ran their solve),
 * "values_product_trans_calls" (successful nkp_values_product_trans* calls), "values_product_trans_us" (wall time of the last one),
 * "trans_index_bytes" (device bytes of the transposed index those calls keep, 0 before the first; part of "device_bytes"),
 * "trans_index_us" (wall time of building it), "trans_index_sent_entries" / "trans_index_recv_entries" (row-distributed: the entries
 * whose products this rank ships to / receives from its peers in every nkp_values_product_trans_dist*; 0 without an index),
 * "residual_batch_calls" (successful nkp_residual_batch* calls), "residual_batch_us" (wall time of the last one),
 * "max_iters" (the iteration cap in force: nkp_options.max_iters or what nkp_set_solve_controls put in its place),
 * "batch_steps" (batched operator
 * applications = lockstep Krylov steps of a group of right-hand sides), "batch_width" (K of the last batched group, 0 if
 * none ran); "batch_member_bytes" (device bytes of the K - 1 further sets of work vectors a batched call has made and keeps:
 * Krylov bases, level vectors, with chained cycles the residual between two cycles; "device_bytes" counts the solver's own set
 * and the K-interleaved buffers, the sum of the two is what the solver holds).  An unknown key returns -1. */
int64_t nkp_get_int (nkp_solver *s, const char *key);

/* New matrix values on the sparsity pattern the solver was created with (the analogue of SuperLU's
 * Fact = SamePattern): val holds nnz values in the CSR order of nkp_create / nkp_create64 (host), d_val the same on
 * the solver's device.  On success every later solve, nkp_spmv and nkp_precond_apply uses the new matrix.
 *   flags = 0: the multilevel hierarchy keeps its coarse cells (the aggregation) and every allocation; all numeric
 *     arrays (twin, Galerkin operators of every level, f32 copies, column factors, coarsest inverse, row scaling) are
 *     recomputed on the device.  They are bit for bit what nkp_create builds from val whenever that create picks the
 *     same coarse cells.  When a coupling the hierarchy dropped as an exact zero becomes non-zero, or a stored one
 *     becomes exactly zero, the refactor notices before writing anything and rebuilds the hierarchy instead.
 *   flags = NKP_REFACTOR_REBUILD: rebuild the hierarchy (coarse cells included) on the new values inside the same
 *     solver; work vectors, stream and the SpMV's row blocks and codes are kept.  Bit for bit nkp_create(val).
 * nkp_get_int: "refactor_count", "refactor_rebuilt" (1 if the last call rebuilt the hierarchy), "refactor_us".
 * Returns 0, NKP_EINVAL (NULL argument, a clone, the row-distributed flavour: use nkp_refactor_dist there, a rebuild
 * while clones are alive),
 * NKP_ESINGULAR (a zero or missing diagonal: the solver is unchanged), NKP_ENOMEM / NKP_EDEVICE.  An error before
 * any value is written leaves the solver solving exactly as before; a zero pivot met while factoring the new values
 * leaves it unusable (every later solve returns NKP_ESINGULAR naming the failed refactor).  No solve may be in
 * flight on the solver or on any of its clones during the call. */
#define NKP_REFACTOR_REBUILD 1
int nkp_refactor (nkp_solver *s, const double *val, int flags);
int nkp_refactor_device (nkp_solver *s, const void *d_val, int flags);

/* nkp_refactor for the row-distributed flavour (nkp_create_dist).  COLLECTIVE: every rank calls it with its own slice.
 * val_loc holds this rank's nnz_loc values in the order of the rowptr_loc / colind_glob it passed to nkp_create_dist (same
 * pattern); d_val_loc is the same array on the solver's device.  flags as for nkp_refactor (0 or NKP_REFACTOR_REBUILD).
 * The reference rebuilds its distributed matrix around pdgssvx (src/solve_ABdist.c:482-483, 539, 571); with these calls a
 * Newton-Krylov driver keeps its solver on every rank and hands it the next Jacobian.
 *   Each rank refreshes its SpMV matrix, its row scaling (equil), its column-block factors (column Jacobi) and its
 *   hierarchy.  The hierarchy's matrix is the diagonal block without overlap, or the [own rows | overlap rows] matrix of
 *   restricted additive Schwarz: the overlap rows' new values come from their owners through ONE alltoallv of device doubles
 *   on the solver's stream.  With flags = 0 the values are recomputed on the kept coarse cells, bit for bit what
 *   nkp_create_dist builds from the new values whenever it picks the same cells; drift in a rank's own or overlap rows, or
 *   NKP_REFACTOR_REBUILD, rebuilds that rank's hierarchy (hierarchies are rank-local, so only the ranks concerned rebuild).
 *   The maps that tie every value to its slot are kept by nkp_create_dist in host memory and uploaded by the first call
 *   (counted in "device_bytes"); after that a device-value call moves no values through the host but the coarsest level's
 *   (dense inverse) and whatever the transport itself stages.
 *   The callbacks of nkp_comm_ops are reached in the same order on every rank (allgather_i64_host, alltoallv when any rank
 *   has overlap rows, allgather_i64_host, allgather_i64_host), whatever path each rank takes locally.
 * nkp_get_int (per rank): "refactor_count", "refactor_rebuilt", "refactor_us", and "refactor_halo_values" (values this rank
 * received in the last call's overlap exchange, 0 without overlap).
 * Returns the codes of nkp_refactor plus NKP_ECOMM, and all ranks agree on success or failure: a rank whose own check fails
 * returns its own code and message (NKP_ESINGULAR for a zero diagonal in its rows, ...), every other rank NKP_ECOMM naming
 * the failed rank.  A failure before the commit point leaves every rank's solver exactly as it was; one after it leaves
 * every rank's solver unusable until a later call succeeds.  A NULL handle or NULL values are refused at once on the calling
 * rank, before any collective.  On a solver nkp_create_dist made for one rank without force_dist (a plain solver) the calls
 * are nkp_refactor / nkp_refactor_device.  No solve may be in flight on the solver during the call. */
int nkp_refactor_dist (nkp_solver *s, const double *val_loc, int flags);
int nkp_refactor_dist_device (nkp_solver *s, const void *d_val_loc, int flags);

/* Use an externally owned HIP stream (hipStream_t cast to void*) instead of the solver's own;
 * NULL = the device's default stream.  The contract (tests/test_gpu_stream_order.py pins it down on a non-blocking stream
 * behind pending work of the caller's):
 *   - every device entry point reads its device operands in order on that stream: work the caller enqueued there before the
 *     call, the producer of an operand included, has run before the library reads anything, and the caller needs no
 *     synchronisation of its own in front of the call.  No operand of the caller's is read on another stream, the null stream
 *     included (where a synchronous copy would run), nor before the stream has reached the call;
 *   - results are complete on return: a device result (X, Y, g, dX) may be read at once from any stream or from the host;
 *   - the batch members of nkp_solve_batch_device* and the transposed handle of nkp_transpose (with its own batch members)
 *     follow the owner's stream, whether they were made before or after this call, and across a refactor that remakes them;
 *   - a clone (nkp_clone) keeps a stream of its own until it is given one with this call;
 *   - the solver must be idle when it is moved: no call in flight on it, on its transposed handle or (row-distributed) on its
 *     peers, and the caller keeps the stream alive for as long as the solver uses it.
 * NKP_EINVAL on a transposed handle: set the stream of the solver it was transposed from. */
int nkp_set_stream (nkp_solver *s, void *hip_stream);

void nkp_destroy (nkp_solver *s);

/* Message of the last failure on this thread ("" if none). */
const char *nkp_last_error (void);

/* ---- row-distributed flavour (one process per GPU, RCCL over xGMI) --------------------- */

/* What the distributed solver needs from the outside world: four collectives.  The library ships
 * an RCCL implementation (nkp_comm_rccl_init); a host program that already owns a communicator
 * (torch.distributed in bench.py, MPI in a port of src/solve_ABdist.c) passes its own callbacks.
 * All callbacks return 0 on success and are called collectively, in the same order, by every rank.
 * This is the stand-in for superlu_gridinit + SuperLU_DIST's internal MPI (src/solve_ABdist.c:461). */
typedef struct nkp_comm_ops {
   void *ctx;
   int rank, nranks;
   /* in-place reduction of `count` doubles in DEVICE memory; op 0 = sum, 1 = max; ordered on hip_stream */
   int (*allreduce) (void *ctx, void *dev_buf, int count, int op, void *hip_stream);
   /* personalised exchange of doubles in DEVICE memory: send_counts[p] values for rank p are taken
    * consecutively from dev_send, recv_counts[p] values from rank p land consecutively in dev_recv */
   int (*alltoallv) (void *ctx, const void *dev_send, const int *send_counts, void *dev_recv, const int *recv_counts, void *hip_stream);
   /* setup only, HOST memory: the same exchange for int32, and an allgather of one int64 per rank */
   int (*alltoallv_i32_host) (void *ctx, const int32_t *send, const int *send_counts, int32_t *recv, const int *recv_counts);
   int (*allgather_i64_host) (void *ctx, int64_t mine, int64_t *all /* nranks */);
} nkp_comm_ops;

/* 128-byte RCCL unique id, created on rank 0 and broadcast by the caller (torch.distributed,
 * MPI or a shared file). */
int nkp_comm_unique_id (void *id128);
/* Fill `ops` with the built-in RCCL implementation (ncclCommInitRank on the current device). */
int nkp_comm_rccl_init (nkp_comm_ops *ops, const void *id128, int rank, int nranks);
void nkp_comm_rccl_free (nkp_comm_ops *ops);
/* Fill `ops` with a host-staged transport over a directory every rank can write (one file per rank and collective).
 * Test-grade: it lets several processes that share ONE GPU run the distributed code path (RCCL needs one GPU per rank).
 * Every blocking read has a deadline (NKP_COMM_TIMEOUT seconds, default 120): a dead peer fails the collective. */
int nkp_comm_file_init (nkp_comm_ops *ops, const char *dir, int rank, int nranks);
void nkp_comm_file_free (nkp_comm_ops *ops);

/* Local row block [fst_row, fst_row + m_loc) with GLOBAL column indices, rowptr rebased to 0
 * -- exactly what dCreate_CompRowLoc_Matrix_dist receives (src/solve_ABdist.c:482-483).
 * blk_start_loc holds the local block offsets (relative to fst_row, blk_start_loc[nblk_loc] =
 * m_loc); a water column must not straddle ranks.  Collective over all ranks.
 * The Krylov iteration is global (halo exchange before every SpMV, one allreduce per
 * Gram-Schmidt pass); the multilevel preconditioner is one hierarchy per rank that, where the cut is
 * lateral (opt->col_i / col_j given), also covers one ring of the neighbouring ranks' water columns
 * (restricted additive Schwarz: setup fetches those rows from their owners through alltoallv_i32_host,
 * every application fetches their residual through alltoallv; NKP_DIST_RAS=0 = diagonal block only).  nkp_solve / nkp_solve_device then take and return the LOCAL slice
 * of b / x, like pdgssvx with ldb = m_loc (src/solve_ABdist.c:571). */
int nkp_create_dist (nkp_solver **out, const nkp_options *opt, int64_t n_global, int64_t fst_row,
                     int64_t m_loc, int64_t nnz_loc, const int32_t *rowptr_loc,
                     const int32_t *colind_glob, const double *val,
                     const int32_t *blk_start_loc, int64_t nblk_loc, int coupled_tracer_cnt,
                     const nkp_comm_ops *comm);

/* Cell-major ordering of a coupled system.  The reference stores coupled tracers tracer-major
 * (src/matrix.c:778-784): cutting such a system into contiguous row blocks (src/solve_ABdist.c:141-144) puts the
 * same-cell coupling entries (src/matrix.c:955-961) off-rank in EVERY row.  In cell-major order -- for every water-column
 * position the columns of all tracers one after the other -- the same contiguous blocks are latitude bands of the whole
 * coupled system, the couplings are rank-local and the halo is the band edge.  Host only, no GPU needed.
 *   nkp_cell_major_order: blk_start[nblk+1] = tracer-major block offsets, nblk = cnt * (blocks per tracer), every tracer
 *     with the same block lengths.  Out: perm[n] (new row -> old row), blk_start_new[nblk+1], col_t[nblk] (tracer of
 *     every new block), col_src[nblk] (old block of every new block: col_i_new[c] = col_i[col_src[c]]).
 *   nkp_permuted_rows: rows [r0, r1) of P A P^T (new numbering on both sides) from the tracer-major CSR; inv[n] = old row
 *     -> new row.  rowptr_loc[r1 - r0 + 1] rebased to 0; colind_loc / val_loc sized for the entries of those rows, columns
 *     sorted ascending within a row. */
int nkp_cell_major_order (int64_t nblk, const int32_t *blk_start, int cnt, int32_t *perm, int32_t *blk_start_new,
                          int32_t *col_t, int32_t *col_src);
int nkp_permuted_rows (int64_t n, const int32_t *rowptr, const int32_t *colind, const double *val, const int32_t *perm,
                       const int32_t *inv, int64_t r0, int64_t r1, int32_t *rowptr_loc, int32_t *colind_loc, double *val_loc);

/* Multi-RHS concurrency: the reference solves its right-hand sides one after the other
 * against one factorisation (RHS loop, src/solve_ABglobal.c:370-409).  nkp_clone gives a second set of work
 * vectors and a second stream on the SAME device-resident matrix, factors and hierarchy (nothing is copied), so
 * that several right-hand sides can be in flight at once: one clone per host thread, each calling nkp_solve /
 * nkp_solve_device on its own handle.  Results are bit-identical to solving on the original.  Destroy clones
 * (nkp_destroy) before the solver they were cloned from.  Single-GPU solvers only.  nkp_refactor on the source
 * without NKP_REFACTOR_REBUILD updates the shared matrix and hierarchy in place, so every clone sees the new values;
 * no solve may then be in flight on any of them.  A refactor that has to rebuild the hierarchy is refused while
 * clones are alive. */
int nkp_clone (nkp_solver *src, nkp_solver **out);

/* Solves with A^T (SuperLU's options.Trans, the mode pdgssvx reads next to Fact and Equil: src/solve_ABglobal.c:327-335) --
 * adjoint tracer problems, sensitivities, the backward pass through a solve.  *out is a solver for A^T on the same device and
 * the same stream as s, built from the matrix s holds ON THE DEVICE (the caller passes no arrays): the CSR is transposed by
 * kernels (rows of A^T sorted by column, stored zeros kept), and the transposed solver is made with the options and tuning s
 * resolved at its creation -- preconditioner, Krylov method, restart, tolerances, equil, precond_steps, the block offsets,
 * col_i / col_j / col_t, coupled_tracer_cnt.  It is bit for bit what nkp_create builds from the host transpose of the same
 * CSR: matrix, every array of the hierarchy, solves and batched solves.  Every entry point keeps its documented meaning on
 * the handle (nkp_solve*, nkp_spmv*: y = A^T x, nkp_precond_apply, nkp_get_int, nkp_ml_level_array, nkp_time_kernel).
 *   Ownership: the handle belongs to s.  A second nkp_transpose (s, ...) returns the same handle.  nkp_destroy (s) destroys
 *   the transposed solver too: it must not be used or destroyed afterwards.  nkp_destroy on the transposed handle itself frees
 *   it and detaches it; a later nkp_transpose builds a new one.  nkp_set_stream (s, ...) moves both solvers.
 *   nkp_refactor / nkp_refactor_device on s keep it in step: after the refactor of s has succeeded the new values are gathered
 *   on the device (valT = val[src], one kernel) and the same sequence runs on the transposed solver with the same flags.  When
 *   the refactor of s fails before its commit point neither solver changes.  When the transposed solver's own refactor fails
 *   it is freed and detached, the call still returns the code of s (one "(rank)" line at verbose >= 1), and the next
 *   nkp_transpose rebuilds from the new matrix and reports its own error.  The transposed solver is not a clone: it does not
 *   block NKP_REFACTOR_REBUILD.  No solve may be in flight on either solver during nkp_transpose or a refactor.
 *   Memory: a second solver (matrix, hierarchy, work vectors) plus the int32 value map, plus nnz doubles from the first
 *   refactor on.  nkp_get_int on s: "trans_device_bytes" (all of that, 0 when there is none; "device_bytes" of s does not
 *   change), "trans_us" (wall time of the last nkp_transpose that built one), "trans_kernel_us" (of which: the device
 *   transpose); on either handle: "is_transpose".
 * Returns 0; NKP_EINVAL with *out = NULL and nothing allocated when s or out is NULL (before any HIP call), s is a clone, s is
 * itself a transposed handle, or s is row-distributed (the transpose of a row block needs an exchange between the ranks:
 * every rank calls nkp_transpose_dist instead);
 * NKP_ESINGULAR when a refactor of s failed after its commit point (s cannot solve either until a refactor succeeds; the message
 * is that failure's); NKP_ENOMEM / NKP_EDEVICE, with s solving exactly as before.  On the transposed handle nkp_refactor*
 * (refactor the solver it was transposed from), nkp_clone and nkp_set_stream return NKP_EINVAL.
 * Cost: one nkp_create plus the device transpose, whose sorting step reads a row of A^T once per entry of that row -- any row
 * length is accepted, but the work is quadratic in it (a column of A with 10^5 entries means 10^10 reads; ocean Jacobians have
 * 5 - 40 per row, a sink that couples a cell to every level a few hundred). */
int nkp_transpose (nkp_solver *s, nkp_solver **out);

/* nkp_transpose for row-distributed solvers.  COLLECTIVE: every rank calls it.  *out is a row-distributed solver for A^T with
 * the row partition of s, on the same device, stream and nkp_comm_ops, built from the row block s holds ON THE DEVICE (the
 * caller passes no arrays).  On every rank it is bit for bit what nkp_create_dist builds from rows [fst_row, fst_row + m_loc)
 * of the host transpose of the global matrix (rows sorted by column, stored zeros kept) with the options and tuning s resolved
 * at its creation, the same local block offsets, col_i / col_j / col_t, coupled_tracer_cnt and comm: the SpMV matrix, the halo
 * plan, every array of every level of the hierarchy -- including the restricted-additive-Schwarz overlap A^T's own pattern asks
 * for, which is generally not A's -- solves and batched solves.  Every entry point keeps its documented meaning on the handle
 * (nkp_solve*, nkp_spmv*: y = A^T x on local slices, nkp_precond_apply, nkp_get_int, nkp_ml_level_array, nkp_gather_root).
 *   How: the rank's m_loc x (m_loc + n_halo) matrix is transposed by the kernels of nkp_transpose; the rows of the result
 *   beyond m_loc are the entries other ranks own, already grouped by destination and sorted by source row.  Their owners know
 *   which of their rows each peer holds as halo (the send rows of the SpMV plan), so only the entry count of each such row, the
 *   global source rows and the values travel; a row of A^T is then the concatenation of the ranks' pieces in rank order, and
 *   kernels place every own and received entry without a sort.  The assembled block goes to the host once and through
 *   nkp_create_dist.
 *   Ownership, as for nkp_transpose: the handle belongs to s; nkp_destroy (s) frees it; nkp_destroy on the handle detaches it;
 *   nkp_set_stream (s, ...) moves both.  The ranks must hold or not hold a handle together: the first thing every call does is
 *   one allgather_i64_host of "I hold a transposed handle".  All hold one: the call returns it, with no further collective.
 *   None does: it is built.  They differ (a rank destroyed its handle alone): every rank returns NKP_EINVAL naming such a rank
 *   and nothing changes; destroy the handle on the other ranks too, then call again.  (A refactor of s in that state is an
 *   error of the caller: the ranks that still hold a handle would wait for the others.)
 *   The callbacks of nkp_comm_ops are reached in the same order on every rank whatever happens locally:
 *     allgather_i64_host   who holds a handle
 *     allgather_i64_host   agreement: local transpose (a broken s -- a refactor that failed after its commit point -- is
 *                          NKP_ESINGULAR here)
 *     alltoallv_i32_host   entry counts of the halo rows, to their owners
 *     allgather_i64_host   agreement: entry counts, receive buffers
 *     alltoallv_i32_host   global source rows of the shipped entries
 *     alltoallv            their values (device doubles, on the solver's stream)
 *     allgather_i64_host   agreement: exchange and placement
 *     nkp_create_dist's own sequence, which succeeds or fails on all ranks together.
 *   After a failed agreement every rank returns: the rank whose step failed its own code and message, the others NKP_ECOMM
 *   naming it.  Either way s solves exactly as before, *out = NULL, and nothing is left allocated.
 *   nkp_refactor_dist / nkp_refactor_dist_device on s keep it in step: after the refactor of s has succeeded on all ranks, the
 *   values of A^T's row block are reassembled on the device (a gather of the values to ship, ONE alltoallv of device doubles on
 *   the solver's stream, a gather into the block's order) and nkp_refactor_dist_device's sequence runs on the transposed solver
 *   with the same flags.  Callbacks after those of the refactor of s: allgather_i64_host (value buffers, allocated at the first
 *   refactor), alltoallv, allgather_i64_host (values), then the sequence of nkp_refactor_dist on the transposed solver.  If any
 *   of this fails on any rank, the agreements tell every rank, and every rank frees and detaches its transposed solver, returns
 *   the code of s and prints one "(rank)" line at verbose >= 1; the next nkp_transpose_dist rebuilds from the new matrix.  A
 *   refactor of s refused before its commit point touches neither solver.
 *   Memory: a second distributed solver, one int32 per entry of A^T's row block (where its value comes from) and per shipped
 *   entry, and, from the first refactor on, doubles for the assembled block, the shipped and the received values.  nkp_get_int
 *   on s: "trans_device_bytes", "trans_us", "trans_kernel_us" (device transpose and placement) as for nkp_transpose,
 *   "trans_sent_entries" / "trans_recv_entries" (entries this rank shipped / received in the last build); on either handle:
 *   "is_transpose".
 * Refused at once on the calling rank, before any collective (NKP_EINVAL): s or out NULL, s a clone, s itself a transposed
 * handle.  On the transposed handle nkp_refactor_dist*, nkp_refactor*, nkp_clone, nkp_set_stream, nkp_transpose and
 * nkp_transpose_dist return NKP_EINVAL without a collective.  On a plain solver (nkp_create, or nkp_create_dist for one rank
 * without force_dist) the call is nkp_transpose.  The ranking step of the device transpose is quadratic in the length of a row
 * of the LOCAL transpose, as in nkp_transpose. */
int nkp_transpose_dist (nkp_solver *s, nkp_solver **out);

/* The sensitivity of a solve to the stored matrix values -- the last step of the backward pass that options.Trans (nkp_transpose
 * above; SuperLU's Trans next to Fact and Equil, src/solve_ABglobal.c:327-335) opens: from x = A^-1 b and the adjoint solution
 * lambda = A^-T (dL/dx) the sensitivity to the right-hand side is lambda itself, and to the matrix it is
 * dL/da_ij = - lambda_i x_j on the sparsity pattern.  For every stored entry e of the solver's CSR matrix, with row i and column
 * j = colind[e], and nrhs pairs of vectors,
 *      s = lambda_0[i] * x_0[j];   s = s + lambda_c[i] * x_c[j]   for c = 1 .. nrhs - 1, ascending;
 *      gval[e] = alpha * s   (accumulate == 0)        gval[e] = gval[e] + alpha * s   (accumulate != 0)
 * in f64, every product and every sum rounded on its own (no fused multiply-add), so the result can be restated bit for bit on
 * the host.  alpha = -1 gives the gradient with respect to the values, in the CSR order of nkp_create / nkp_create64 -- the order
 * in which nkp_refactor* take new values.
 *   Buffers, all the caller's: lambda and x hold nrhs vectors of n doubles, column-major, vector c at offset c * ld, ld >= n, as in
 *   nkp_solve_batch_device; gval holds nnz doubles and is read only when accumulate != 0.  nkp_value_gradient takes host buffers,
 *   nkp_value_gradient_device buffers on the solver's device.  1 <= nrhs <= 8; with more pairs call again with accumulate = 1:
 *   the sum then chains per CALL, gval = (gval + alpha * s_first) + alpha * s_second, which in general is not the bit pattern of
 *   one longer sum.  The work runs on the solver's stream and has finished when the call returns.
 *   Only the pattern is read: the call is allowed on a clone, on a solver whose refactor failed after its commit point, and on
 *   a transposed handle, where it gives the gradient with respect to the values of A^T in A^T's own CSR order (rows sorted by
 *   column).  Work space -- K-interleaved copies of lambda and x for nrhs >= 2, the device staging of the host flavour -- is
 *   allocated at first use, kept, and counted in "device_bytes"; a failed allocation leaves the solver exactly as it was.
 *   nkp_get_int: "value_gradient_calls", "value_gradient_us" (wall time of the last call).
 * Row-distributed solvers (nkp_create_dist with more than one rank, or force_dist): the same two entry points, COLLECTIVE, with
 * the same nrhs on every rank.  Each rank passes its own rows of every vector (ld >= m_loc) and receives nnz_loc values in the
 * order of the rowptr_loc / colind_glob it created the solver with.  lambda is needed on the own rows only; the halo rows of x
 * come from their owners, all nrhs vectors in ONE alltoallv of nrhs-wide rows (for nrhs >= 2 the K-wide buffers of the batched
 * solve, K = 2, 4 or 8; counted in "dist_alltoallv_calls").  The callbacks of nkp_comm_ops are reached in the same order on
 * every rank whatever happens locally:
 *      allgather_i64_host   agreement: arguments (nrhs, ld), work space, staging of the host vectors
 *      alltoallv            the halo rows of x (device doubles, on the solver's stream; made like the SpMV's, also when this
 *                           rank sends and receives nothing)
 *      allgather_i64_host   agreement: exchange and kernel
 *   After a failed agreement every rank returns: the rank whose step failed its own code and message, the others NKP_ECOMM
 *   naming it; gval is then undefined, the solvers solve as before.
 * Returns 0; NKP_EINVAL for a NULL solver or buffer (refused on the calling rank before the solver is looked at and before any
 * collective; the message names the argument), nrhs outside 1 .. 8 or ld < n (found before any HIP call; on a row-distributed
 * solver told to the other ranks through the first agreement); NKP_ENOMEM / NKP_EDEVICE; NKP_ECOMM. */
int nkp_value_gradient_device (nkp_solver *s, int nrhs, const void *d_lambda, const void *d_x, int64_t ld, double alpha, int accumulate, void *d_gval);
int nkp_value_gradient (nkp_solver *s, int nrhs, const double *lambda, const double *x, int64_t ld, double alpha, int accumulate, double *gval);

/* The product of caller-supplied values on the solver's sparsity pattern with nrhs vectors -- the forward-mode partner of
 * nkp_value_gradient: with dA the perturbation of the stored values, the tangent of X = A^-1 B is dX = A^-1 (dB - dA X), and
 * dA X is this product.  It also gives A_new x and b - A_new x for the next Jacobian on the same stencil before a refactor.
 * For every row i and vector c, with t_c[i] = the sum over the stored entries e of row i of val[e] * x_c[colind[e]],
 *      y_c[i] = alpha * t_c[i]   (accumulate == 0; y is not read and may hold anything)      y_c[i] = y_c[i] + alpha * t_c[i]   (accumulate != 0)
 * alpha * t is one rounded product, the sum one rounded sum (no fused multiply-add).  t_c[i] has the bits nkp_spmv_device gives
 * for x_c on a solver created from the same pattern with val as its values: +0.0, then every stored entry of the row in stored
 * order, each product and each sum rounded on its own; a row of more than 2048 entries is summed in the SpMV's tree for such
 * rows.  The bits are the same for every nrhs.  A row without entries gets alpha * (+0.0).
 *   Buffers, all the caller's: val holds nnz doubles in the CSR order of nkp_create / nkp_create64 (the order of nkp_refactor* and
 *   nkp_value_gradient*); x and y hold nrhs vectors, column-major, vector c at offset c * ldx and c * ldy, ldx, ldy >= n; rows
 *   n .. ld - 1 are neither read nor written.  1 <= nrhs <= 8.  nkp_values_product takes host buffers, nkp_values_product_device
 *   buffers on the solver's device.  y == x is refused (NKP_EINVAL); any other overlap of y with val or x is the caller's error
 *   and gives undefined values.  The work runs on the solver's stream and has finished when the call returns.
 *   Only the pattern is read: the call is allowed on a clone, on a solver whose refactor failed after its commit point, and on a
 *   transposed handle, where val is in A^T's own CSR order and t is the product with A^T's pattern; a refactor does not change
 *   the result.  Work space -- the K-interleaved copy of x for nrhs >= 2 (8 K n bytes, K = 2, 4 or 8), the device staging of the
 *   host flavour (8 (nnz + 2 nrhs n) bytes) -- is allocated at first use, all or nothing, kept, and counted in "device_bytes"; a
 *   failed allocation leaves the solver exactly as it was.  nkp_get_int: "values_product_calls", "values_product_us".
 * Row-distributed solvers: the same entry points, COLLECTIVE, with the same nrhs on every rank.  Each rank passes nnz_loc values
 * in the order of the rowptr_loc / colind_glob it created the solver with and its own rows of every vector (ldx, ldy >= m_loc).
 * The halo rows of x come from their owners, all nrhs vectors in ONE alltoallv (K = 1: the SpMV's buffers; K >= 2: the K-wide
 * buffers of the batched solve; counted in "dist_alltoallv_calls").  The callbacks are reached in the same order on every rank
 * whatever happens locally, the sequence of nkp_value_gradient*:
 *      allgather_i64_host   agreement: arguments, work space, staging of the host arrays
 *      alltoallv            the halo rows of x (always made, also by a rank that sends and receives nothing)
 *      allgather_i64_host   agreement: exchange and kernel
 *   After a failed agreement every rank returns: the rank whose step failed its own code and message, the others NKP_ECOMM
 *   naming it; y is then undefined, the solvers solve as before.
 * Returns 0; NKP_EINVAL for a NULL solver or buffer (refused on the calling rank before the solver is looked at and before any
 * collective; the message names the argument), nrhs outside 1 .. 8, ldx or ldy < n, y == x (found before any HIP call; on a
 * row-distributed solver told to the other ranks through the first agreement); NKP_ENOMEM / NKP_EDEVICE; NKP_ECOMM. */
int nkp_values_product_device (nkp_solver *s, int nrhs, const void *d_val, const void *d_x, int64_t ldx, double alpha, int accumulate, void *d_y, int64_t ldy);
int nkp_values_product (nkp_solver *s, int nrhs, const double *val, const double *x, int64_t ldx, double alpha, int accumulate, double *y, int64_t ldy);

/* The same product with the TRANSPOSED pattern, the values staying in A's order: with G the matrix that holds val on A's
 * pattern, y_c (+)= alpha * G^T x_c.  nkp_value_gradient is bilinear in (lambda, x); its derivative with respect to lambda is a
 * nkp_values_product, its derivative with respect to x is this product -- with it the solve, the transposed solve, the gradient and
 * the two products are closed under differentiation (second and higher derivatives through a solve; torch_op.py).
 * For every column j of A and vector c, t_c[j] starts at +0.0 and adds val[e] * x_c[row of e] over the stored entries e with
 * colind[e] == j in ascending order of (row, stored position), each product and each sum rounded on its own (no fused
 * multiply-add); then
 *      y_c[j] = alpha * t_c[j]   (accumulate == 0; y is not read and may hold anything)      y_c[j] = y_c[j] + alpha * t_c[j]   (accumulate != 0)
 * t_c has the bits nkp_spmv_device gives for x_c on a solver created from the host transpose of (pattern, val), taken stably (an
 * entry of A^T's row j keeps its place among the entries of A in row-major order: repeated and unsorted entries of A have a
 * defined place); a column of more than 2048 entries is summed in the SpMV's tree for such rows.  The bits are the same for every
 * nrhs.  A column of A without entries gets alpha * (+0.0).
 *   Buffers as for nkp_values_product: val holds nnz doubles in the CSR order of nkp_create (NOT transposed by the caller); x and
 *   y hold nrhs vectors, vector c at c * ldx and c * ldy, ldx, ldy >= n, rows n .. ld - 1 neither read nor written; 1 <= nrhs <=
 *   8; y == x is refused.  nkp_values_product_trans takes host buffers, nkp_values_product_trans_device buffers on the solver's
 *   device.  The work runs on the solver's stream and has finished when the call returns.
 *   The transposed index: the first call builds, on the device, the pattern of A^T (4 (n + 1) + 4 nnz bytes), the map from its
 *   entries to A's (4 nnz bytes) and its row blocks -- the blocks a solver created from the host transpose has -- and the solver
 *   keeps them: "trans_index_bytes", "trans_index_us", counted in "device_bytes".  While it is built the device transpose holds
 *   16 nnz + 4 n bytes more. All or nothing: a failed allocation (NKP_ENOMEM) leaves the solver exactly as it was.  A refactor keeps
 *   the pattern, with or without NKP_REFACTOR_REBUILD, so the index survives it.  The index is the solver's own: it neither uses nor
 *   feeds a handle from nkp_transpose, and a solver that has both holds 8 nnz + 4 (n + 1) bytes twice.  Work space beyond it is
 *   that of nkp_values_product, the same buffers (the K-interleaved copy of x, the staging of the host flavour).
 *   Only the pattern is read: the call is allowed on a solver whose refactor failed after its commit point.
 * Refused with NKP_EINVAL, the solver solving exactly as before: a clone (call it on the solver it was cloned from, as for
 * nkp_transpose); a transposed handle (call it on its owner; on the handle nkp_values_product multiplies with A^T's pattern and
 * values in A^T's order); a row-distributed solver, force_dist included -- the product sends products back to the owners of their
 * columns, a collective of its own: nkp_values_product_trans_dist* below -- refused on the calling rank without any collective.  A
 * NULL solver or buffer is refused on the
 * calling thread before the solver is looked at, the message names the argument; nrhs outside 1 .. 8, ldx or ldy < n, y == x
 * are found before any HIP call.  NKP_ENOMEM / NKP_EDEVICE.  nkp_get_int: "values_product_trans_calls", "values_product_trans_us". */
int nkp_values_product_trans_device (nkp_solver *s, int nrhs, const void *d_val, const void *d_x, int64_t ldx, double alpha, int accumulate, void *d_y, int64_t ldy);
int nkp_values_product_trans (nkp_solver *s, int nrhs, const double *val, const double *x, int64_t ldx, double alpha, int accumulate, double *y, int64_t ldy);

/* The same product on a row-distributed solver: y_c (+)= alpha * G^T x_c, G the global matrix that holds every rank's values on the
 * global pattern.  COLLECTIVE, with the same nrhs (1 .. 8) on every rank.  val_loc holds this rank's nnz_loc values in the order of
 * the rowptr_loc / colind_glob it gave nkp_create_dist; x and y hold this rank's own rows of every vector, vector c at c * ldx and
 * c * ldy, ldx, ldy >= m_loc, rows m_loc .. ld - 1 neither read nor written; y == x is refused.  For the own columns j,
 * y_c[j] (+)= alpha * t_c[j] with t_c[j] as for nkp_values_product_trans: it starts at +0.0 and adds val[e] * x_c[row of e] over ALL
 * stored entries of global column j, whichever rank stores them, in ascending (global row, stored position) order, each product
 * and each sum rounded on its own; a column of more than 2048 entries is summed in the SpMV's tree.  Each rank's slice of y has
 * the bits nkp_values_product_trans_device gives on a single-GPU solver of the whole matrix, whatever the number of ranks.
 *   How: with a row partition "ascending global row" is rank 0's contributions, then rank 1's, ...  The PRODUCTS travel, not partial
 *   sums: for every entry in one of its halo columns a rank ships val[e] * x_c[row of e] (one rounded product per vector) to the
 *   owner of the column, 8 * K * (entries shipped) bytes per call (K = 1, 2, 4, 8 the interleave width that serves nrhs); the owner
 *   walks the assembled row of G^T in order and adds own and received products alike, one rounded add each.
 *   The transposed index is built collectively at the first call and kept: the local transpose of this rank's [own | halo]
 *   rectangle (on the device, as nkp_transpose_dist makes it), the entry count of every halo row to its owner, and the placement
 *   of every contribution; no source rows and no values travel.  Kept on the device, "trans_index_bytes": 4 (m_loc + 1) bytes of
 *   row offsets, 8 bytes per assembled entry (own + received: where its value and its x row are), the row blocks, 8 bytes per
 *   shipped entry.  All or nothing ACROSS ranks: if any rank could not build its part, every rank frees what it built and the
 *   solvers are exactly as before.  The index survives nkp_refactor_dist*, with or without NKP_REFACTOR_REBUILD, and neither uses
 *   nor feeds a handle from nkp_transpose_dist.  "trans_index_sent_entries" / "trans_index_recv_entries" count what this rank ships
 *   and receives.  Work space: [ own rows | received products ] x K and the K-wide send buffer, made at first use for the K asked
 *   for, grown when a wider K comes, counted in "device_bytes"; the host flavour stages val_loc, x and y like nkp_values_product.
 *   Refused with NKP_EINVAL when 8 * (entries shipped or received) does not fit the int counts of the exchange.
 * The callbacks, in this order on every rank whatever happens locally:
 *      allgather_i64_host   agreement: arguments (nrhs, ldx, ldy, y != x), work space, staging; without an index also the local transpose
 *    [ alltoallv_i32_host   entry counts of the halo rows        -- only in a call that builds the index ]
 *    [ allgather_i64_host   agreement: placement, index, commit  -- only in a call that builds the index ]
 *      alltoallv            the products (always made, also by a rank that ships and receives nothing; "dist_alltoallv_calls")
 *      allgather_i64_host   agreement: exchange and kernel
 * After a failed agreement every rank returns: the failing rank its own code and message, the others NKP_ECOMM naming it; y is
 * undefined and the solvers solve as before.  Refused on the calling rank before any collective, NKP_EINVAL: a NULL solver or
 * buffer (the message names the argument); a clone; a transposed handle (call it on its owner).  On a plain solver -- from
 * nkp_create, or from nkp_create_dist for one rank without force_dist -- the calls ARE nkp_values_product_trans*; with force_dist on
 * one rank the distributed path runs with empty exchanges.  nkp_get_int as on a single-GPU solver: "values_product_trans_calls",
 * "values_product_trans_us", "trans_index_bytes", "trans_index_us". */
int nkp_values_product_trans_dist_device (nkp_solver *s, int nrhs, const void *d_val_loc, const void *d_x, int64_t ldx, double alpha, int accumulate, void *d_y,
                                          int64_t ldy);
int nkp_values_product_trans_dist (nkp_solver *s, int nrhs, const double *val_loc, const double *x, int64_t ldx, double alpha, int accumulate, double *y, int64_t ldy);

/* The tangent (forward mode) of a solve: dX = A^-1 (dB - dA X) for nrhs right-hand sides, device buffers.  R_c = dB_c - dA X_c is
 * formed in work space of the solver (8 nrhs ld bytes, at first use, kept, counted in "device_bytes") and has the bits of
 * nkp_values_product_device (s, nrhs, d_dval, d_x, ldx, -1.0, 1, R, ld) on a copy of dB; then nkp_solve_batch_device (s, nrhs, R,
 * d_dx, ld, berr, iters, relres) runs, so dX, iters, relres, berr and the return code are that call's: the tangent solve converges
 * or fails like any solve.  d_db == NULL means dB = 0; d_dval == NULL means no dA term (d_x may then be NULL, no product is made);
 * both NULL is NKP_EINVAL.  d_x: the nrhs solutions X (vector c at c * ldx), d_db and d_dx: vector c at c * ld; d_dx may be d_db.
 * Row-distributed solvers: collective; the sequence above (its first agreement always, the exchange and the second agreement
 * only with d_dval), then the batched solve's own collectives.  Every rank must pass d_dval NULL or non-NULL alike: the first
 * agreement carries it, and a mismatch is NKP_EINVAL on every rank, naming a rank, before any exchange.
 * nkp_get_int: "tangent_calls".  Errors as for nkp_values_product_device (NULL s, d_dx, or d_x with d_dval: refused before the
 * handle is read). */
int nkp_solve_tangent_device (nkp_solver *s, int nrhs, const void *d_dval, const void *d_x, int64_t ldx, const void *d_db, void *d_dx, int64_t ld,
                              double *berr, int *iters, double *relres);

/* How good are nrhs given solutions under the matrix the handle solves with now?  For every column c, from ONE pass over A:
 *      r_c = b_c - A x_c (stored in R when R is not NULL),   rnorm[c] = sqrt (sum_i r_c[i]^2),   bnorm[c] = sqrt (sum_i b_c[i]^2),
 *      berr[c] = max_i |r_c[i]| / (|A||x_c| + |b_c|)[i]      -- the componentwise backward error the solves report.
 * An inexact Newton driver asks this first after every nkp_refactor*: the forcing term needs ||b - A x|| and ||b||, and a column
 * whose old solution is still good enough needs no solve.  The call does not judge convergence and returns 0 on success: relres =
 * rnorm / bnorm is the caller's to form (bnorm may be 0).
 *   Per row i and column c the pass keeps t = +0.0; t += val[e] * x_c[colind[e]] and d = +0.0; d += fabs (val[e] * x_c[colind[e]])
 *   over the stored entries of the row in stored order, every product and every sum rounded on its own (no fused multiply-add): the
 *   bits of nkp_spmv_device and of the |A||x| pass of the solves; a row of more than 2048 entries is summed in the SpMV's tree for
 *   such rows, t and d alike.  Then r = b - t, den = d + fabs (b) and q = fabs (r) / den, where den == 0 gives q = 0 for r == 0 and
 *   1e300 otherwise, and a NaN of r or den (or Inf / Inf) gives NaN.  berr[c] is the maximum of q, NaN sticky: it has the bits of the
 *   berr nkp_solve_device reports for the same x and b.  r^2 and b^2 are one rounded product each; they are summed per CSR row block
 *   of A in a fixed tree and the row blocks in a fixed order, so rnorm and bnorm depend on A's pattern alone: the same bits for
 *   every nrhs, every position of a vector among the columns, and every repetition of the call.  No atomics.
 *   A is read from its CSR values, never from per-column diagonals (tuning spmv_diag): a padded slot times a non-finite x would
 *   differ, and the check is meant for suspect vectors.  A non-finite entry of x_c or b_c makes that column's numbers NaN or Inf by
 *   the rules above, does not disturb the other columns, and is not an error.
 *   Which matrix: the one the handle solves with now -- after nkp_refactor* the new values; the unscaled system whatever equil is
 *   (the row scaling of the row-weighted iteration is applied to vectors, A's values are never stored scaled); on a transposed
 *   handle A^T.  A clone is allowed and reads the shared matrix.  A solver whose refactor failed after its commit point is refused
 *   like the solves (NKP_ESINGULAR).
 *   Buffers: B, X and R hold nrhs vectors, column-major, vector c at c * ldb, c * ldx and c * ldr, every ld >= n; rows n .. ld - 1
 *   are neither read nor written and columns behind nrhs are untouched.  1 <= nrhs <= 8 (more vectors: call again).  R may be NULL
 *   (no residual is stored; ldr is then ignored).  R == X is refused, because other rows still gather x; R == B with ldr == ldb is
 *   allowed (every row reads its b before its r is written); any other overlap of R with B or X is the caller's error.  rnorm,
 *   bnorm and berr are host arrays of nrhs doubles each, or NULL; asking for nothing (R and all three NULL) is refused.
 *   nkp_residual_batch takes host buffers, nkp_residual_batch_device buffers on the solver's device; B and X are not modified.
 *   The work runs on the solver's stream (nkp_set_stream), reads the caller's operands in order on that stream and has finished
 *   when the call returns.  Compulsory bytes: 12 nnz + 4 (n + 1) + 16 nrhs n, plus 8 nrhs n when R is written.
 *   Work space -- the K-interleaved copy of X for nrhs >= 2 (8 K n bytes, K = 2, 4 or 8), the partial sums (24 K bytes per row
 *   block of A), the device staging of the host flavour (8 nrhs n bytes each for B, X and, when asked for, R) -- is allocated at
 *   first use, all or nothing, kept, and counted in "device_bytes"; a failed allocation leaves the solver exactly as it was.
 *   nkp_get_int: "residual_batch_calls" (successful calls), "residual_batch_us" (wall time of the last one).
 * Row-distributed solvers: the same entry points, COLLECTIVE, with the same nrhs on every rank; each rank passes its own rows of
 * every vector (every ld >= m_loc) and gets its own rows of R; rnorm, bnorm and berr are global and identical on all ranks (berr
 * with the bits of a single-GPU solver of the whole matrix; what the transport's max makes of a NaN is the transport's business,
 * as for nkp_solve).  The callbacks, in this order on every rank:
 *      allgather_i64_host   agreement: arguments, work space, staging of the host arrays
 *      alltoallv            the halo rows of X, K wide, in ONE exchange (always made; "dist_alltoallv_calls")
 *      allreduce (sum)      2 K doubles: the squared norms            ("dist_allreduce_calls")
 *      allreduce (max)      K doubles: the backward errors            ("dist_allreduce_calls")
 *      allgather_i64_host   agreement: exchange, kernel, reductions
 *   A rank whose own arguments or work space fail still makes the first agreement; when it fails every rank returns after it --
 *   the failing rank its own code and message, the others NKP_ECOMM naming it -- and nothing else is exchanged.  Once the first
 *   agreement has passed, the remaining four callbacks are reached on every rank whatever happens locally, and the second
 *   agreement tells a local failure to all in the same way.  The outputs are then undefined; the solvers solve as before.  On a
 *   plain solver there is no collective.
 * Returns 0; NKP_EINVAL for a NULL solver, B or X (refused on the calling rank before the solver is looked at and before any
 * collective; the message names the argument), nrhs outside 1 .. 8, an ld < n, R == X, nothing asked for (found before any HIP
 * call; on a row-distributed solver told to the other ranks through the first agreement); NKP_ESINGULAR; NKP_ENOMEM / NKP_EDEVICE;
 * NKP_ECOMM. */
int nkp_residual_batch_device (nkp_solver *s, int nrhs, const void *d_B, int64_t ldb, const void *d_X, int64_t ldx,
                               void *d_R, int64_t ldr, double *rnorm, double *bnorm, double *berr);
int nkp_residual_batch        (nkp_solver *s, int nrhs, const double *B, int64_t ldb, const double *X, int64_t ldx,
                               double *R, int64_t ldr, double *rnorm, double *bnorm, double *berr);

/* hipSetDevice for host programs that do not link HIP themselves (call before nkp_comm_rccl_init). */
int nkp_set_device (int device);

/* Collective: concatenate every rank's local slice (host, m_loc doubles) in rank order into
 * x_global (host, n_global doubles, significant on rank 0 only) -- what put_B_dist does with
 * MPI_Send/MPI_Recv tag 4 (src/solve_ABdist.c:377, 406). */
int nkp_gather_root (nkp_solver *s, const double *x_loc, double *x_global);

/* The whole host-side plan of nkp_create_dist as an object, for tests without a GPU: collective over the ranks through the
 * HOST callbacks of `comm` (alltoallv_i32_host, allgather_i64_host); no HIP call.  Fields (nkp_dist_plan_size gives the
 * element count, nkp_dist_plan_copy copies): SpMV side -- "colind_ext" (int32, the local columns renumbered [own | halo]),
 * "halo_rows" (global rows received before every SpMV; with grid positions in opt the halo is completed to whole water
 * columns), "send_rows" (own rows sent, grouped by destination), "need" / "give" (per-rank counts); hierarchy side, filled
 * when the overlap is on (nkp_dist_plan_size (p, "ras") == 1) -- the matrix on [own rows | overlap rows]: "rowptr",
 * "colind", "val" (double), "blk_start", "col_i", "col_j", "col_t", and "sel_hpos" (position in the halo of every overlap row, -1
 * for rows of ring 2 and beyond, which the SpMV never reads).  The overlap rows follow the own rows in ascending global row order.
 * "ras_rings" (size only) is the depth the ranks agreed on (0 without overlap); with two or more rings the overlap residual has
 * an exchange of its own: "ras_send_rows" (own local rows sent, grouped by destination, ascending within each), "ras_need" /
 * "ras_give" (per-rank row counts; the rows from rank p arrive in hierarchy order).  What nkp_refactor_dist redoes the values
 * from: "origin" (per entry of "colind": the own local entry it comes from, or -1 - position in the received overlap values),
 * "ship" (own local entries shipped, grouped by destination), "ent_need" / "ent_give" (per-rank entry counts).
 * "smooth_exchange" (size only) is 1 when the ranks agreed on the fine-level exchange (tuning dist_smooth_exchange) and there is an
 * overlap; then, per colour c = (i + j) % 2 of the water columns: "smooth_send_rows0" / "1" (own local rows that other ranks hold
 * as overlap rows, all rings, grouped by destination, ascending within each), "smooth_give0" / "1" and "smooth_need0" / "1"
 * (per-rank row counts; the rows from rank p arrive in the hierarchy order of this rank's overlap rows of that colour), and
 * "smooth_recv_rows0" / "1" (those overlap rows as rows of the hierarchy's matrix).  All of them are empty otherwise. */
typedef struct nkp_dist_plan nkp_dist_plan;
int nkp_dist_overlap_plan_host (nkp_dist_plan **out, const nkp_options *opt, int64_t n_global, int64_t fst_row, int64_t m_loc,
                                int64_t nnz_loc, const int32_t *rowptr_loc, const int32_t *colind_glob, const double *val,
                                const int32_t *blk_start_loc, int64_t nblk_loc, int coupled_tracer_cnt, const nkp_comm_ops *comm);
int64_t nkp_dist_plan_size (const nkp_dist_plan *p, const char *what);
int nkp_dist_plan_copy (const nkp_dist_plan *p, const char *what, void *dst);
void nkp_dist_plan_free (nkp_dist_plan *p);

/* Host-only planning step of nkp_create_dist, exposed so the partition / halo logic can be tested
 * without a GPU: given this rank's rows and the row offsets of all ranks (starts[nranks+1]),
 * writes the remapped column indices (local rows -> [0, m_loc), halo -> m_loc + position in the
 * sorted list of needed off-rank rows) into colind_ext[nnz_loc], the needed global rows into
 * halo_rows (capacity nnz_loc; *n_halo entries used) and how many come from each rank into
 * need_counts[nranks].  Returns 0 or NKP_EINVAL. */
int nkp_dist_plan_host (int64_t m_loc, int64_t nnz_loc, const int32_t *rowptr_loc, const int32_t *colind_glob,
                        int rank, int nranks, const int64_t *starts, int32_t *colind_ext, int32_t *halo_rows,
                        int64_t *n_halo, int32_t *need_counts);

/* Introspection of the multilevel hierarchy as it sits on the device (tests: the levels the setup kernels build must equal
 * the ones the host routines build, entry for entry).  Copies one array of level `level` (0 = finest) to dst and returns its
 * element count (dst == NULL: the count only); negative = error.  what: "rowptr" (int32, rows + 1), "colind" (int32),
 * "valf" (float, the f32 storage of a level operator) / "val" (double, where the f64 values are kept), "cmap" (int32: row ->
 * row of the next level), "rptr" / "ridx" (int32: row of the next level -> its rows here), "blk_start" (int32), "fac"
 * (double, band factors of the column blocks), "perm0" (int32, level 0: row -> original row), "coarse_inv" (double, last
 * level, empty when that level is relaxed instead), "color_blk" (int32, 3 entries, every level with column blocks -- a last
 * level that is relaxed included: column blocks [color_blk[c], color_blk[c + 1]) have colour c, so the rows of colour 0 are
 * [0, blk_start[color_blk[1]]); a host array, copied without a device call), "col_kernel" (int32, 11 entries, every level with
 * column blocks, a host array like "color_blk": which column-solve kernels serve the level -- wave_columns, wave_fused, stream,
 * ldsres (0 / 1 = LDS-resident / 2 = packed), gw (columns per group), P (half bandwidth stored), dropped (1 if entries beyond
 * the band were dropped), max_len (longest column), gs_ok (the fused half sweep can serve the level), ngrp, lds_doubles (dynamic
 * LDS of the lane kernels, in doubles)), "dg_ptr" (int32, columns + 1) / "dg_key" (int32) / "dg_voff" (int64, columns) / "dg_val"
 * (float): the per-column diagonals of tuning ml_diag, empty when the level runs on CSR -- column c of blk_start, of len rows, has
 * the keys dg_key[dg_ptr[c] .. dg_ptr[c + 1]), ascending, and its row kl has the entry dg_val[dg_voff[c] + s * len + kl] in column
 * key_s + kl, 0 where it has none; "dg_gptr" (int32, columns + 1) / "dg_grp" (int32 pairs): the groups of consecutive keys the
 * residual kernel loads x for once -- column c has the groups dg_gptr[c] .. dg_gptr[c + 1], in slot order, group g with the first
 * key dg_grp[2 g] and dg_grp[2 g + 1] = s0 | m << 16, its first slot in the column and its keys (m <= 5 and m <= 64 - rows + 1,
 * rows = ceil (len / ceil (len / 64)), the column's tallest tile); "wave_diag" (int32, 1 entry, a host value): 1 where the level's
 * wave-fused half sweeps read these diagonals (gs_wave_diag_kernel), 0 where they read CSR or the level is not wave-fused;
 * "lane_diag" (int32, 1 entry, a host value): 1 where the half sweeps of a lane-per-column level are one launch each on these
 * diagonals (gs_lanes_diag_kernel, tuning ml_lane_fused), and then "grp_tile" (int32, ngrp * gw): per lane of every packed group
 * the column it holds, counted in columns that have rows, -1 = none.  All in the level's colour-major row order. */
int64_t nkp_ml_level_array (nkp_solver *s, int level, const char *what, void *dst, int64_t capacity_bytes);

/* The same for the per-column diagonals of the solver's own matrix A (tuning spmv_diag), in the row order and with the water
 * columns of nkp_create: what = "dg_ptr", "dg_key", "dg_voff", "dg_gptr", "dg_grp" as above, "dg_val" (double).  Every array is
 * empty when A runs on CSR (spmv_diag = 0, not eligible, no blk_start, row-distributed, a transposed handle).  A clone reads its
 * owner's.  Also A's CSR arrays as the device holds them, "rowptr" (n + 1), "colind" (nnz), "val" (nnz, double) -- the caller's
 * stored order; on a transposed handle the device transpose --, and "fac" (double, (2 P + 1) n), the band factors of
 * NKP_PRECOND_COLUMN_JACOBI (empty under any other preconditioner). */
int64_t nkp_matrix_array (nkp_solver *s, const char *what, void *dst, int64_t capacity_bytes);

/* Host-only planning step of the multilevel preconditioner inside nkp_create, exposed so the aggregation logic can
 * be tested without a GPU: builds the low-order twin, the coarse cells of every level (geometric groups split by
 * lateral connectivity) and the Galerkin products, and reports
 *   *n_levels, rows[l] (l < *n_levels), and for every level l < *n_levels - 1, concatenated in level order:
 *   cmap   : coarse row (level l+1 numbering) of every row of level l            (sum of rows[0 .. n_levels-2] entries)
 *   col_of : column block of every row of level l+1                              (sum of rows[1 .. n_levels-1] entries)
 * `capacity` bounds both output arrays (entries).  col_i / col_j as in nkp_options.  Returns 0, NKP_EINVAL, or NKP_ENOMEM
 * when the capacity is too small. */
int nkp_ml_plan_host (int64_t n, const int32_t *rowptr, const int32_t *colind, const double *val, const int32_t *blk_start,
                      int64_t nblk, const int32_t *col_i, const int32_t *col_j, int coupled_tracer_cnt, int max_levels,
                      int coarsest_rows, int64_t capacity, int *n_levels, int64_t *rows, int32_t *cmap, int32_t *col_of);

#ifdef __cplusplus
}
#endif
#endif
