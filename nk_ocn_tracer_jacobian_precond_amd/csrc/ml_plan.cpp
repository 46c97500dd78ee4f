// Host planner of the multilevel water-column preconditioner (NKP_PRECOND_MULTILEVEL): which rows form the coarse cells of
// every level, and the level operators in the order the device holds them.  Plain C++, no HIP call: multilevel.hip uploads
// and factors what this unit returns, mlsetup.hip builds the large levels of the same hierarchy with kernels.
//
// Why it exists: with exact water-column blocks alone, restarted GMRES needs >1e4 iterations
// on upwind3/centred Jacobians at 3 degrees and stalls outright at 1 degree (SURVEY.md section 7,
// hard part 1) -- which is why the reference uses a sparse direct solver
// (src/solve_ABglobal.c:353).  This preconditioner keeps the column-block kernel of colblock.hip
// as its smoother and adds the two things the block-Jacobi sweep lacks:
//
//  1. a monotone low-order twin L of A: every wrong-signed coupling BETWEEN water columns is
//     removed by symmetric artificial diffusion d_ij = max(0, -a_ij, -a_ji) (algebraic
//     upwinding: centred / upwind3 advection weights, src/matrix.c:1239-1273, 1610-1690, become
//     the donor-cell operator; the +-isopycnal cross terms, :881-930, become positive); entries
//     inside a column stay exact.  -L is an M-matrix, so column-block Gauss-Seidel converges on
//     it and on every Galerkin coarsening of it.
//  2. a hierarchy: columns are aggregated pairwise twice (~4 columns per aggregate, levels k
//     kept), P is piecewise constant, L_{l+1} = P^T L_l P; every level keeps the "contiguous
//     water column" layout, so the SAME wave-per-column kernels run on all levels.  Columns are
//     2-coloured and stored colour-major, so a Gauss-Seidel half-sweep is one row-range
//     residual SpMV + one block-range column solve.
//
// One V(nu,nu) cycle (mlcycle.hip) approximates L^-1; FGMRES (krylov.hip) iterates on the original A.
#include "ml_plan.h"

#include <math.h>
#include <stdio.h>

#include <array>
#include <atomic>
#include <chrono>
#include <memory>
#include <numeric>

namespace mlp {
namespace {

// ---------------------------------------------------------------- low-order twin
// L = A + D - diag(rowsum D), D_ij = max(0, -a_ij, -a_ji) for i, j in different columns.  Rows are sorted by column, so
// a_ji is found by bisection in row j (no transpose); three row-parallel passes: new values and kept-entry counts,
// prefix sum, fill.  Entries whose coupling becomes exactly zero are not stored.
void build_low_order (int64_t n, const int *rowptr, const int *colind, const double *val, const std::vector<int> &col_of, int threads, HostCsr &L)
{
   const int64_t nnz = rowptr[n];
   RawDoubles nv;
   nv.resize ((size_t) nnz);
   std::vector<int> keep ((size_t) n + 1, 0);
   for_row_chunks (n, threads, [&] (int, int64_t r0, int64_t r1) {
      for (int64_t i = r0; i < r1; i++) {
         double dsum = 0.0;
         int diag_pos = -1, cnt = 0;
         for (int e = rowptr[i]; e < rowptr[i + 1]; e++) {
            const int j = colind[e];
            double a = val[e];
            if (j == i) { diag_pos = e; nv[e] = a; cnt++; continue; }
            if (col_of[j] != col_of[i]) {
               const int *lo = colind + rowptr[j], *hi = colind + rowptr[j + 1];
               const int *q = std::lower_bound (lo, hi, (int) i);
               const double aji = (q < hi && *q == (int) i) ? val[q - colind] : 0.0;
               double d = 0.0;
               if (-a > d) d = -a;
               if (-aji > d) d = -aji;
               a += d;
               dsum += d;
            }
            nv[e] = a;
            if (a != 0.0 || col_of[j] == col_of[i]) cnt++;          // in-column entries are always stored
         }
         if (diag_pos >= 0) nv[diag_pos] -= dsum;
         keep[(size_t) i + 1] = cnt;
      }
   });
   L.n = n;
   L.rowptr.assign ((size_t) n + 1, 0);
   for (int64_t i = 0; i < n; i++) L.rowptr[(size_t) i + 1] = L.rowptr[(size_t) i] + keep[(size_t) i + 1];
   L.colind.resize ((size_t) L.rowptr[(size_t) n]);
   L.val.resize ((size_t) L.rowptr[(size_t) n]);
   for_row_chunks (n, threads, [&] (int, int64_t r0, int64_t r1) {
      for (int64_t i = r0; i < r1; i++) {
         int q = L.rowptr[(size_t) i];
         for (int e = rowptr[i]; e < rowptr[i + 1]; e++) {
            const int j = colind[e];
            if (j != i && col_of[j] != col_of[i] && nv[e] == 0.0) continue;
            L.colind[(size_t) q] = j;
            L.val[(size_t) q] = nv[e];
            q++;
         }
      }
   });
}

// ---------------------------------------------------------------- column graph helpers
struct ColGraph {
   std::vector<int> ptr, nbr;
   std::vector<double> w;
};

void build_col_graph (const HostCsr &L, const std::vector<int> &blk_start, const std::vector<int> &col_of, ColGraph &G)
{
   const int ncol = (int) blk_start.size () - 1;
   G.ptr.assign (ncol + 1, 0);
   G.nbr.clear ();
   G.w.clear ();
   std::vector<double> acc (ncol, 0.0);
   std::vector<int> touched;
   for (int c = 0; c < ncol; c++) {
      touched.clear ();
      for (int r = blk_start[c]; r < blk_start[c + 1]; r++)
         for (int e = L.rowptr[r]; e < L.rowptr[r + 1]; e++) {
            const int c2 = col_of[L.colind[e]];
            if (c2 == c) continue;
            if (acc[c2] == 0.0) touched.push_back (c2);
            acc[c2] += fabs (L.val[e]) + 1.0e-300;
         }
      std::sort (touched.begin (), touched.end ());
      for (int c2 : touched) {
         G.nbr.push_back (c2);
         G.w.push_back (acc[c2]);
         acc[c2] = 0.0;
      }
      G.ptr[c + 1] = (int) G.nbr.size ();
   }
}

// one pass of pairwise matching on a weighted graph; returns group id per node (ordered by first member)
int pairwise_match (int nn, const std::vector<int> &ptr, const std::vector<int> &nbr, const std::vector<double> &w, std::vector<int> &group)
{
   group.assign (nn, -1);
   int ng = 0;
   for (int c = 0; c < nn; c++) {
      if (group[c] >= 0) continue;
      int best = -1;
      double bw = 0.0;
      for (int q = ptr[c]; q < ptr[c + 1]; q++)
         if (group[nbr[q]] < 0 && nbr[q] != c && w[q] > bw) { bw = w[q]; best = nbr[q]; }
      group[c] = ng;
      if (best >= 0) group[best] = ng;
      ng++;
   }
   return ng;
}

// collapse a node graph onto groups
void collapse_graph (int nn, int ng, const std::vector<int> &group, const ColGraph &G, ColGraph &H)
{
   std::vector<std::vector<int>> members (ng);
   for (int c = 0; c < nn; c++) members[group[c]].push_back (c);
   H.ptr.assign (ng + 1, 0);
   H.nbr.clear ();
   H.w.clear ();
   std::vector<double> acc (ng, 0.0);
   std::vector<int> touched;
   for (int g = 0; g < ng; g++) {
      touched.clear ();
      for (int c : members[g])
         for (int q = G.ptr[c]; q < G.ptr[c + 1]; q++) {
            const int g2 = group[G.nbr[q]];
            if (g2 == g) continue;
            if (acc[g2] == 0.0) touched.push_back (g2);
            acc[g2] += G.w[q];
         }
      std::sort (touched.begin (), touched.end ());
      for (int g2 : touched) {
         H.nbr.push_back (g2);
         H.w.push_back (acc[g2]);
         acc[g2] = 0.0;
      }
      H.ptr[g + 1] = (int) H.nbr.size ();
   }
}

// greedy 2-colouring: each column takes the colour its already-coloured neighbours use least (by weight)
void two_colour (int ncol, const ColGraph &G, std::vector<int> &colour)
{
   colour.assign (ncol, -1);
   for (int c = 0; c < ncol; c++) {
      double w0 = 0.0, w1 = 0.0;
      for (int q = G.ptr[c]; q < G.ptr[c + 1]; q++) {
         const int k = colour[G.nbr[q]];
         if (k == 0) w0 += G.w[q];
         else if (k == 1) w1 += G.w[q];
      }
      colour[c] = (w0 <= w1) ? 0 : 1;
      if (w0 == 0.0 && w1 == 0.0) colour[c] = 0;
   }
}

// ---------------------------------------------------------------- split aggregates (geometric groups, connectivity-aware)
// A group of columns (2 x 2 or 4 x 4 in (i, j)) is NOT turned into one coarse column blindly: at every depth k the
// members that are wet at k form one coarse cell per CONNECTED set (lateral couplings of the level operator between
// members), because a piecewise-constant cell over mutually uncoupled water (two sides of a ridge, a deep pocket
// next to open water) cannot represent the near-kernel of the operator -- it is constant per connected piece, not per
// group -- and neither the column smoother nor any coarser level then removes that error (measured: the two-grid
// iteration with an exact coarse solve needs 88 Krylov steps at a 0.25-degree cell Courant number, 21 with the split).
//  * same-depth connected sets of at most `pocket` cells are merged into one coarse cell even across groups (a deep
//    pocket is a strongly coupled cluster hanging on weak vertical diffusion: it must become ONE unknown);
//  * the sets are threaded through depth into coarse columns: the child set with the largest overlap continues its
//    parent's column, every other child starts a stub column (first depth > 0) at the same (i, j);
//  * a stub of the fine level that no outside row feels (every coupling into it is < tau x that row's diagonal) is a
//    leaf: the column solve makes it follow its neighbours exactly, so it is absorbed into the coarse cell it hangs
//    from instead of surviving as an unknown on every coarser level.
// Rows keep their depth: row r of column c sits at depth ktop[c] + (r - blk_start[c]).
struct SplitResult {
   std::vector<int> cmap;                     // fine row -> coarse row
   std::vector<int> blk_start, ktop, gi, gj, gt;   // coarse columns
   int absorbed = 0, stubs = 0;
};

// Lock-free union-find (several host threads unite concurrently): a root is only ever linked under a LOWER index with a
// compare-and-swap, so the final root of every set is its lowest row whatever the interleaving -- the partition and the
// numbering derived from it are deterministic.
struct UnionFind {
   std::unique_ptr<std::atomic<int>[]> p;
   size_t n;
   explicit UnionFind (size_t n_) : p (n_ ? new std::atomic<int>[n_] : nullptr), n (n_)
   {
      for (size_t i = 0; i < n; i++) p[i].store ((int) i, std::memory_order_relaxed);
   }
   int find (int x)
   {
      for (;;) {
         const int px = p[x].load (std::memory_order_relaxed);
         if (px == x) return x;
         const int gp = p[px].load (std::memory_order_relaxed);
         if (gp != px) { int expect = px; p[x].compare_exchange_weak (expect, gp, std::memory_order_relaxed); }   // path halving
         x = px;
      }
   }
   void unite (int a, int b)
   {
      for (;;) {
         a = find (a);
         b = find (b);
         if (a == b) return;
         if (a > b) std::swap (a, b);                              // link the higher root b under the lower root a
         int expect = b;
         if (p[b].compare_exchange_strong (expect, a, std::memory_order_relaxed)) return;
      }
   }
};

void split_aggregate (const HostCsr &L, const std::vector<int> &blk_start, const std::vector<int> &col_of, const std::vector<int> &ktop,
                      const std::vector<int> &group, const std::vector<int> &ggi, const std::vector<int> &ggj, const std::vector<int> &ggt,
                      const std::vector<int> &col_t, const PlanKnobs &K, SplitResult &R)
{
   const int64_t n = L.n;
   const int ncol = (int) blk_start.size () - 1;
   const int pocket = K.pocket, threads = K.threads;
   const double theta = K.theta, tau = K.tau;
   const bool timing = K.times;
   auto tick0 = std::chrono::steady_clock::now ();
   auto lap = [&] (const char *what) {
      if (!timing) return;
      auto now = std::chrono::steady_clock::now ();
      printf ("   split_aggregate (%lld rows): %-28s %.3f s\n", (long long) n, what, std::chrono::duration<double> (now - tick0).count ());
      tick0 = now;
   };
   auto depth = [&] (int r) { const int c = col_of[r]; return ktop[c] + (r - blk_start[c]); };
   auto row_at = [&] (int c, int k) -> int { const int r = blk_start[c] + (k - ktop[c]); return (k >= ktop[c] && r < blk_start[c + 1]) ? r : -1; };
   // per row: strongest lateral coupling (only needed for a threshold theta > 0); per column: how strongly any outside
   // row of the same tracer feels it, and its own strongest coupling (only needed where stub columns exist)
   bool have_stubs = false;
   for (int c = 0; c < ncol && !have_stubs; c++) have_stubs = ktop[c] > 0;
   std::vector<double> diag, rowmax, felt, best;
   std::vector<int> anchor (ncol, -1);
   std::vector<char> dang (ncol, 0);
   if (theta > 0.0) {
      rowmax.assign (n, 0.0);
      for (int64_t r = 0; r < n; r++)
         for (int e = L.rowptr[r]; e < L.rowptr[r + 1]; e++) {
            const int c2 = col_of[L.colind[e]];
            if (c2 != col_of[r] && col_t[c2] == col_t[col_of[r]]) rowmax[r] = std::max (rowmax[r], fabs (L.val[e]));
         }
   }
   if (have_stubs && tau > 0.0) {
      diag.assign (n, 0.0);
      felt.assign (ncol, 0.0);
      best.assign (ncol, -1.0);
      for (int64_t r = 0; r < n; r++)
         for (int e = L.rowptr[r]; e < L.rowptr[r + 1]; e++)
            if (L.colind[e] == r) diag[r] = fabs (L.val[e]);
      for (int64_t r = 0; r < n; r++) {
         const int c = col_of[r];
         for (int e = L.rowptr[r]; e < L.rowptr[r + 1]; e++) {
            const int j = L.colind[e], c2 = col_of[j];
            if (c2 == c || col_t[c2] != col_t[c]) continue;
            if (ktop[c2] == 0 && ktop[c] == 0) continue;                // neither end is a stub
            const double v = fabs (L.val[e]);
            const double f = diag[r] > 0.0 ? v / diag[r] : 1.0e300;
            if (f > felt[c2]) felt[c2] = f;
            if (v >= best[c]) { best[c] = v; anchor[c] = j; }          // strongest coupling of the column, ties -> later entry
         }
      }
      for (int c = 0; c < ncol; c++) dang[c] = (ktop[c] > 0 && felt[c] < tau && anchor[c] >= 0);
      std::vector<char> bad (ncol, 0);
      for (int c = 0; c < ncol; c++) bad[c] = dang[c] && dang[col_of[anchor[c]]];
      for (int c = 0; c < ncol; c++) if (bad[c]) dang[c] = 0;
   }
   lap ("stub analysis");
   // lateral edges between cells of the same depth, united on the fly: U0 over all of them (it finds the small same-depth
   // sets = pockets), U over the edges inside a group; a second scan of the pockets' rows adds their cross-group edges to U
   UnionFind U (n), U0 (pocket > 0 ? n : 0);
   auto scan_row = [&] (int64_t r, auto &&visit) {
      const int c = col_of[r];
      if (dang[c]) return;
      const int k = depth ((int) r);
      for (int e = L.rowptr[r]; e < L.rowptr[r + 1]; e++) {
         const int j = L.colind[e], c2 = col_of[j];
         if (c2 == c || dang[c2] || col_t[c2] != col_t[c]) continue;
         const int dk = depth (j) - k;
         if (dk < -1 || dk > 1) continue;
         if (theta > 0.0 && fabs (L.val[e]) < theta * rowmax[r]) continue;
         const int t = row_at (c2, k);
         if (t >= 0) visit ((int) r, t, group[c] == group[c2]);
      }
   };
   for_row_chunks (n, threads, [&] (int, int64_t r0, int64_t r1) {
      for (int64_t r = r0; r < r1; r++)
         scan_row (r, [&] (int a, int b, bool same) {
            if (pocket > 0) U0.unite (a, b);
            if (same) U.unite (a, b);
         });
   });
   if (pocket > 0) {
      std::vector<int> root0 (n), size (n, 0);
      for_row_chunks (n, threads, [&] (int, int64_t r0, int64_t r1) { for (int64_t r = r0; r < r1; r++) root0[r] = U0.find ((int) r); });
      for (int64_t r = 0; r < n; r++) size[root0[r]]++;
      for_row_chunks (n, threads, [&] (int, int64_t r0, int64_t r1) {
         for (int64_t r = r0; r < r1; r++)
            if (size[root0[r]] <= pocket && size[root0[r]] > 1)
               scan_row (r, [&] (int a, int b, bool same) { if (!same) U.unite (a, b); });
      });
   }
   lap ("union-find over the edges");
   // components numbered in order of their lowest row
   std::vector<int> comp (n, -1);
   int ncomp = 0;
   for (int64_t r = 0; r < n; r++) {
      const int root = U.find ((int) r);
      if (comp[root] < 0) comp[root] = ncomp++;       // root is the lowest row of its set, so it is met first
      comp[r] = comp[root];
   }
   std::vector<int> kcomp (ncomp, 0);
   for (int64_t r = 0; r < n; r++) kcomp[comp[r]] = depth ((int) r);
   lap ("component numbering");
   // overlaps between a set and the sets directly below it: the pairs (set of row r, set of the row below r) are bucketed
   // by parent with a counting sort (set ids are dense), every bucket -- the handful of rows of one set -- is sorted and
   // its runs counted
   std::vector<int> bestpar (ncomp, -1), bestpar_cnt (ncomp, 0), bestchi (ncomp, -1), bestchi_cnt (ncomp, 0);
   {
      std::vector<int> bptr ((size_t) ncomp + 1, 0);
      for (int c = 0; c < ncol; c++)
         for (int r = blk_start[c]; r + 1 < blk_start[c + 1]; r++) bptr[(size_t) comp[r] + 1]++;
      for (int q = 0; q < ncomp; q++) bptr[(size_t) q + 1] += bptr[(size_t) q];
      std::vector<int> child ((size_t) bptr[(size_t) ncomp]);
      {
         std::vector<int> fill (bptr.begin (), bptr.end () - 1);
         for (int c = 0; c < ncol; c++)
            for (int r = blk_start[c]; r + 1 < blk_start[c + 1]; r++) child[(size_t) fill[(size_t) comp[r]]++] = comp[r + 1];
      }
      // parents in ascending id, children ascending inside a bucket: a strict '>' keeps the lowest id on ties, like the
      // sorted list of pairs did
      for (int par = 0; par < ncomp; par++) {
         int *b0 = child.data () + bptr[(size_t) par], *b1 = child.data () + bptr[(size_t) par + 1];
         if (b1 - b0 > 1) std::sort (b0, b1);
         for (int *q = b0; q < b1;) {
            int *q2 = q;
            while (q2 < b1 && *q2 == *q) q2++;
            const int chi = *q, cnt = (int) (q2 - q);
            if (cnt > bestpar_cnt[chi]) { bestpar_cnt[chi] = cnt; bestpar[chi] = par; }
            if (cnt > bestchi_cnt[par]) { bestchi_cnt[par] = cnt; bestchi[par] = chi; }
            q = q2;
         }
      }
   }
   lap ("overlap pairs (buckets)");
   // coarse columns: sets in order of depth (counting sort), then of id
   std::vector<int> order (ncomp);
   {
      int kmax = 0;
      for (int q = 0; q < ncomp; q++) kmax = std::max (kmax, kcomp[q]);
      std::vector<int> kptr ((size_t) kmax + 2, 0);
      for (int q = 0; q < ncomp; q++) kptr[(size_t) kcomp[q] + 1]++;
      for (int k = 0; k <= kmax; k++) kptr[(size_t) k + 1] += kptr[(size_t) k];
      for (int q = 0; q < ncomp; q++) order[(size_t) kptr[(size_t) kcomp[q]]++] = q;
   }
   std::vector<int> ccol (ncomp, -1), cc_ktop, cc_len;
   for (int id : order) {
      const int par = bestpar[id];
      if (par >= 0 && bestchi[par] == id) {
         ccol[id] = ccol[par];
         cc_len[ccol[id]]++;
      } else {
         ccol[id] = (int) cc_ktop.size ();
         cc_ktop.push_back (kcomp[id]);
         cc_len.push_back (1);
      }
   }
   lap ("threading");
   // absorbed stubs own no coarse column: drop the (now empty) columns their sets opened
   const int nraw = (int) cc_ktop.size ();
   // a coarse column sits at the (i, j) of the group of its lowest fine row (a merged pocket can span groups)
   std::vector<char> used (nraw, 0);
   std::vector<int> cc_group (nraw, 0);
   for (int64_t r = 0; r < n; r++)
      if (!dang[col_of[r]] && !used[ccol[comp[r]]]) { used[ccol[comp[r]]] = 1; cc_group[ccol[comp[r]]] = group[col_of[r]]; }
   std::vector<int> newid (nraw, -1);
   int ncc = 0;
   for (int q = 0; q < nraw; q++) if (used[q]) newid[q] = ncc++;
   R.blk_start.assign (ncc + 1, 0);
   R.ktop.resize (ncc); R.gi.resize (ncc); R.gj.resize (ncc); R.gt.resize (ncc);
   for (int q = 0; q < nraw; q++) {
      if (!used[q]) continue;
      const int a = newid[q];
      R.blk_start[a + 1] = cc_len[q];
      R.ktop[a] = cc_ktop[q];
      R.gi[a] = ggi[cc_group[q]]; R.gj[a] = ggj[cc_group[q]]; R.gt[a] = ggt[cc_group[q]];
      if (cc_ktop[q] > 0) R.stubs++;
   }
   for (int a = 0; a < ncc; a++) R.blk_start[a + 1] += R.blk_start[a];
   R.cmap.assign (n, -1);
   for (int64_t r = 0; r < n; r++) {
      if (dang[col_of[r]]) continue;
      const int a = newid[ccol[comp[r]]];
      R.cmap[r] = R.blk_start[a] + (depth ((int) r) - R.ktop[a]);
   }
   lap ("coarse columns and map");
   for (int c = 0; c < ncol; c++) {
      if (!dang[c]) continue;
      R.absorbed++;
      const int target = R.cmap[anchor[c]];
      for (int r = blk_start[c]; r < blk_start[c + 1]; r++) R.cmap[r] = target;
   }
}

// the inverse of a map fine row -> coarse row: the fine rows of coarse row I are ridx[rptr[I] .. rptr[I + 1]), ascending
void rows_of_coarse (const std::vector<int> &cmap, int64_t nc, std::vector<int> &rptr, std::vector<int> &ridx)
{
   const int64_t n = (int64_t) cmap.size ();
   rptr.assign (nc + 1, 0);
   ridx.resize (n);
   for (int64_t i = 0; i < n; i++) rptr[cmap[i] + 1]++;
   for (int64_t I = 0; I < nc; I++) rptr[I + 1] += rptr[I];
   std::vector<int> fill (rptr.begin (), rptr.end () - 1);
   for (int64_t i = 0; i < n; i++) ridx[fill[cmap[i]]++] = (int) i;
}

// Galerkin product with a piecewise-constant P given as fine row -> coarse row
void galerkin (const HostCsr &L, const std::vector<int> &cmap, int64_t nc, int threads, HostCsr &C)
{
   std::vector<int> rptr, ridx;
   rows_of_coarse (cmap, nc, rptr, ridx);
   // coarse rows in parallel: every thread owns a contiguous run of coarse rows, with its own accumulator over the
   // coarse columns, and appends to its own output; the pieces are stitched together in row order
   C.n = nc;
   C.rowptr.assign (nc + 1, 0);
   const int nt_max = threads;
   std::vector<std::vector<int>> pc (nt_max);
   std::vector<std::vector<double>> pv (nt_max);
   std::vector<int64_t> first (nt_max, 0), last (nt_max, 0);
   for_row_chunks (nc, threads, [&] (int t, int64_t I0, int64_t I1) {
      first[t] = I0;
      last[t] = I1;
      std::vector<double> acc (nc, 0.0);
      std::vector<char> mark (nc, 0);
      std::vector<int> touched;
      std::vector<int> &oc = pc[t];
      std::vector<double> &ov = pv[t];
      oc.reserve ((size_t) ((L.colind.size () / 2) * (double) (I1 - I0) / (double) (nc ? nc : 1)) + 16);
      ov.reserve (oc.capacity ());
      for (int64_t I = I0; I < I1; I++) {
         touched.clear ();
         for (int q = rptr[I]; q < rptr[I + 1]; q++) {
            const int i = ridx[q];
            for (int e = L.rowptr[i]; e < L.rowptr[i + 1]; e++) {
               const int J = cmap[L.colind[e]];
               if (!mark[J]) { mark[J] = 1; touched.push_back (J); }
               acc[J] += L.val[e];
            }
         }
         std::sort (touched.begin (), touched.end ());
         int cnt = 0;
         for (int J : touched) {
            if (acc[J] != 0.0 || J == I) {
               oc.push_back (J);
               ov.push_back (acc[J]);
               cnt++;
            }
            acc[J] = 0.0;
            mark[J] = 0;
         }
         C.rowptr[I + 1] = cnt;
      }
   });
   for (int64_t I = 0; I < nc; I++) C.rowptr[I + 1] += C.rowptr[I];
   C.colind.resize ((size_t) C.rowptr[nc]);
   C.val.resize ((size_t) C.rowptr[nc]);
   {
      // every piece into its place, one thread per piece (the destination pages are first touched here)
      std::vector<std::thread> pool;
      for (int t = 0; t < nt_max; t++) {
         if (last[t] <= first[t]) continue;
         pool.emplace_back ([&, t] () {
            std::copy (pc[t].begin (), pc[t].end (), C.colind.begin () + C.rowptr[first[t]]);
            std::copy (pv[t].begin (), pv[t].end (), C.val.begin () + C.rowptr[first[t]]);
         });
      }
      for (std::thread &th : pool) th.join ();
   }
}

}  // namespace

bool dense_inverse (int n, std::vector<double> &a /* row-major n*n, overwritten by its inverse */)
{
   std::vector<double> inv ((size_t) n * n, 0.0);
   for (int i = 0; i < n; i++) inv[(size_t) i * n + i] = 1.0;
   for (int k = 0; k < n; k++) {
      int p = k;
      double mx = fabs (a[(size_t) k * n + k]);
      for (int i = k + 1; i < n; i++)
         if (fabs (a[(size_t) i * n + k]) > mx) { mx = fabs (a[(size_t) i * n + k]); p = i; }
      if (!(mx > 0.0)) return false;
      if (p != k)
         for (int c = 0; c < n; c++) {
            std::swap (a[(size_t) k * n + c], a[(size_t) p * n + c]);
            std::swap (inv[(size_t) k * n + c], inv[(size_t) p * n + c]);
         }
      const double piv = 1.0 / a[(size_t) k * n + k];
      for (int c = 0; c < n; c++) { a[(size_t) k * n + c] *= piv; inv[(size_t) k * n + c] *= piv; }
      for (int i = 0; i < n; i++) {
         if (i == k) continue;
         const double f = a[(size_t) i * n + k];
         if (f == 0.0) continue;
         double *ai = &a[(size_t) i * n], *ak = &a[(size_t) k * n], *ii = &inv[(size_t) i * n], *ik = &inv[(size_t) k * n];
         for (int c = 0; c < n; c++) { ai[c] -= f * ak[c]; ii[c] -= f * ik[c]; }
      }
   }
   a.swap (inv);
   return true;
}

PlanKnobs plan_knobs (const nkp_tuning &t)
{
   PlanKnobs k;
   k.split = t.ml_split != 0;
   k.pocket = t.ml_pocket;
   k.theta = t.ml_theta;
   k.tau = t.ml_tau;
   k.big_from = t.ml_big_from;
   k.huge_from = t.ml_huge_from;
   k.threads = setup_thread_count (t);
   k.times = t.plan_times != 0;
   return k;
}

void init_first_nat (Nat &N, int64_t n, const int *rowptr, const int *colind, const double *val, const int *blk_start_in, int64_t nblk,
                     const int *col_i, const int *col_j, const int *col_t, int tracer_cnt, bool with_twin, const PlanKnobs &K, SetupTimes &T)
{
   using clk = std::chrono::steady_clock;
   N.blk_start.assign (blk_start_in, blk_start_in + nblk + 1);
   N.ktop.assign (nblk, 0);
   if (with_twin) {
      N.col_of.resize (n);
      for (int64_t c = 0; c < nblk; c++)
         for (int r = N.blk_start[c]; r < N.blk_start[c + 1]; r++) N.col_of[r] = (int) c;
      auto t0 = clk::now ();
      build_low_order (n, rowptr, colind, val, N.col_of, K.threads, N.L);
      T.low += std::chrono::duration<double> (clk::now () - t0).count ();
   }
   if (col_i && col_j) {
      N.gi.assign (col_i, col_i + nblk);
      N.gj.assign (col_j, col_j + nblk);
      N.gt.resize (nblk);
      const int64_t per = (tracer_cnt > 1 && nblk % tracer_cnt == 0) ? nblk / tracer_cnt : nblk;
      // tracer of a column: positional (tracer-major rows, src/matrix.c:778-784) unless the caller names it -- the
      // distributed flavour appends the neighbouring ranks' overlap columns behind its own
      for (int64_t c = 0; c < nblk; c++) N.gt[c] = col_t ? col_t[c] : (int) (c / per);
   }
}

int geo_groups (const Nat &N, int sh, std::vector<int> &agg, std::vector<int> &cgi, std::vector<int> &cgj, std::vector<int> &cgt)
{
   const int ncol = (int) N.blk_start.size () - 1;
   std::vector<std::pair<std::array<int, 3>, int>> sorted (ncol);
   for (int c = 0; c < ncol; c++) sorted[c] = { { N.gt[c], N.gj[c] >> sh, N.gi[c] >> sh }, c };
   std::sort (sorted.begin (), sorted.end ());
   std::vector<int> gid_sorted (ncol), first_member;
   int ng = 0;
   for (int q = 0; q < ncol; q++) {
      if (q == 0 || sorted[q].first != sorted[q - 1].first) { first_member.push_back (sorted[q].second); ng++; }
      gid_sorted[sorted[q].second] = ng - 1;
   }
   // renumber groups by their first (lowest natural index) member so coarse columns keep the j, i order
   std::vector<int> order (ng);
   std::iota (order.begin (), order.end (), 0);
   std::sort (order.begin (), order.end (), [&] (int a, int b) { return first_member[a] < first_member[b]; });
   std::vector<int> newid (ng);
   for (int q = 0; q < ng; q++) newid[order[q]] = q;
   agg.resize (ncol);
   cgi.resize (ng); cgj.resize (ng); cgt.resize (ng);
   for (int c = 0; c < ncol; c++) {
      const int a = newid[gid_sorted[c]];
      agg[c] = a;
      cgi[a] = N.gi[c] >> sh; cgj[a] = N.gj[c] >> sh; cgt[a] = N.gt[c];
   }
   return ng;
}

// 2 x 2 groups on the big levels, 4 x 4 from level 3 down: every kernel of a small level runs at its latency
// floor, so fewer small levels pay (1 degree: 8 -> 6 levels, +5 % iterations, -14 % cycle time);
// NKP_ML_BIG_FROM=l moves the switch, -1 disables it (from level 2 it costs +68 % iterations)
// (round 2, with the connectivity-aware cells and omega = 1.1: grids of fewer than 200 000 columns per tracer
// keep the switch at level 3 -- 1 degree: 64 iterations / 0.21 s either way -- larger grids coarsen 2 x 2 all the
// way, where the better hierarchy outweighs two more latency-bound levels: 0.5 degree 92 -> 79 iterations,
// 0.95 -> 0.81 s; 0.25 degree 129 -> 105, 4.1 -> 3.4 s)
int group_shift (const PlanKnobs &K, int level, int ncol_level0, int tracer_cnt)
{
   int bf = K.big_from;
   if (bf == -3) bf = ncol_level0 / (tracer_cnt > 0 ? tracer_cnt : 1) >= 200000 ? -1 : 3;
   if (K.huge_from >= 0 && level >= K.huge_from) return 3;          // 8 x 8 groups (A/B knob ml_huge_from)
   return (bf >= 0 && level >= bf) ? 2 : 1;
}

void colour_major_columns (Nat &N, std::vector<int> &newstart)
{
   const int ncol = (int) N.blk_start.size () - 1;
   newstart.assign (ncol, 0);
   N.pblk.clear ();
   N.pblk.reserve (ncol + 1);
   N.pblk.push_back (0);
   N.ncol0 = 0;
   for (int pass = 0; pass < 2; pass++)
      for (int c = 0; c < ncol; c++)
         if (N.colour[c] == pass) {
            if (pass == 0) N.ncol0++;
            newstart[c] = N.pblk.back ();
            N.pblk.push_back (N.pblk.back () + (N.blk_start[c + 1] - N.blk_start[c]));
         }
}

void extend_nat_levels (std::vector<Nat> &nat, int level0, int ncol_level0, int tracer_cnt, int max_levels, int coarsest_rows, int verbose, int rank,
                        const PlanKnobs &K, SetupTimes &T)
{
   using clk = std::chrono::steady_clock;
   auto secs = [] (clk::time_point a) { return std::chrono::duration<double> (clk::now () - a).count (); };
   double &t_graph = T.graph, &t_galerkin = T.galerkin;
   for (int l = (int) nat.size () - 1;; l++) {
      Nat &N = nat[l];
      const int ncol = (int) N.blk_start.size () - 1;
      ColGraph G;
      const bool geo = !N.gi.empty ();
      if (!geo) { auto t0 = clk::now (); build_col_graph (N.L, N.blk_start, N.col_of, G); t_graph += secs (t0); }
      if (geo) {
         N.colour.resize (ncol);
         for (int c = 0; c < ncol; c++) N.colour[c] = (N.gi[c] + N.gj[c]) & 1;
      } else
         two_colour (ncol, G, N.colour);
      // colour-major permutation of rows
      std::vector<int> newstart;
      colour_major_columns (N, newstart);
      N.perm.resize (N.L.n);
      N.inv.resize (N.L.n);
      for (int c = 0; c < ncol; c++)
         for (int r = N.blk_start[c]; r < N.blk_start[c + 1]; r++) {
            N.inv[r] = newstart[c] + (r - N.blk_start[c]);
            N.perm[N.inv[r]] = r;
         }

      const bool last = (level0 + l + 1 >= max_levels) || (N.L.n <= coarsest_rows) || ncol <= 4;
      if (last) break;
      int n2 = 0;
      N.agg.resize (ncol);
      std::vector<int> cgi, cgj, cgt;
      if (geo) {
         n2 = geo_groups (N, group_shift (K, level0 + l, ncol_level0, tracer_cnt), N.agg, cgi, cgj, cgt);
      } else {
         // two passes of pairwise matching -> aggregates of up to 4 columns
         std::vector<int> g1, g2;
         const int n1 = pairwise_match (ncol, G.ptr, G.nbr, G.w, g1);
         ColGraph G1;
         collapse_graph (ncol, n1, g1, G, G1);
         n2 = pairwise_match (n1, G1.ptr, G1.nbr, G1.w, g2);
         for (int c = 0; c < ncol; c++) N.agg[c] = g2[g1[c]];
      }
      N.nagg = n2;
      Nat C;
      int64_t ncr = 0;
      if (geo && K.split) {
         // connectivity-aware coarse cells inside the geometric groups (see split_aggregate)
         auto t0 = clk::now ();
         SplitResult R;
         split_aggregate (N.L, N.blk_start, N.col_of, N.ktop, N.agg, cgi, cgj, cgt, N.gt, K, R);
         t_graph += secs (t0);
         ncr = R.blk_start.back ();
         if (ncr >= N.L.n) break;                       // no coarsening possible
         if (verbose)
            printf ("(%d) multilevel: level %d -> %d: %d columns in %d groups -> %d coarse columns (%d stubs), %d leaf stubs absorbed\n", rank, level0 + l, level0 + l + 1, ncol, n2,
                    (int) R.blk_start.size () - 1, R.stubs, R.absorbed);
         n2 = (int) R.blk_start.size () - 1;
         N.cmap.swap (R.cmap);
         C.blk_start.swap (R.blk_start);
         C.ktop.swap (R.ktop);
         C.gi.swap (R.gi); C.gj.swap (R.gj); C.gt.swap (R.gt);
      } else {
         if (n2 >= ncol) break;                         // no coarsening possible
         // coarse columns: length = longest member
         std::vector<int> clen (n2, 0);
         for (int c = 0; c < ncol; c++) clen[N.agg[c]] = std::max (clen[N.agg[c]], N.blk_start[c + 1] - N.blk_start[c]);
         C.gi.swap (cgi); C.gj.swap (cgj); C.gt.swap (cgt);
         C.blk_start.assign (n2 + 1, 0);
         C.ktop.assign (n2, 0);
         for (int a = 0; a < n2; a++) C.blk_start[a + 1] = C.blk_start[a] + clen[a];
         ncr = C.blk_start[n2];
         N.cmap.resize (N.L.n);
         for (int c = 0; c < ncol; c++)
            for (int r = N.blk_start[c]; r < N.blk_start[c + 1]; r++) N.cmap[r] = C.blk_start[N.agg[c]] + (r - N.blk_start[c]);
      }
      { auto t0 = clk::now (); galerkin (N.L, N.cmap, ncr, K.threads, C.L); t_galerkin += secs (t0); }
      C.col_of.resize (ncr);
      for (int a = 0; a < n2; a++)
         for (int r = C.blk_start[a]; r < C.blk_start[a + 1]; r++) C.col_of[r] = a;
      nat.push_back (std::move (C));
   }
}

void colour_major_operator (const Nat &N, int threads, ColourMajorLevel &P)
{
   const int64_t nl = N.L.n;
   P.prow.assign (nl + 1, 0);
   P.pcol.resize (N.L.colind.size ());              // sized without a fill: the row-parallel loop below writes every entry
   P.pval.resize (N.L.colind.size ());
   for (int64_t i = 0; i < nl; i++) P.prow[i + 1] = P.prow[i] + (N.L.rowptr[N.perm[i] + 1] - N.L.rowptr[N.perm[i]]);
   for_row_chunks (nl, threads, [&] (int, int64_t i0, int64_t i1) {
      std::vector<std::pair<int, double>> tmp;
      for (int64_t i = i0; i < i1; i++) {
         const int o = N.perm[i];
         tmp.clear ();
         for (int e = N.L.rowptr[o]; e < N.L.rowptr[o + 1]; e++) tmp.emplace_back (N.inv[N.L.colind[e]], N.L.val[e]);
         std::sort (tmp.begin (), tmp.end ());
         int q = P.prow[i];
         for (auto &t : tmp) { P.pcol[q] = t.first; P.pval[q] = t.second; q++; }
      }
   });
}

void colour_major_transfers (const Nat &N, const Nat &C, ColourMajorLevel &P)
{
   const int64_t nl = N.L.n;
   P.cmap.resize (nl);
   for (int64_t i = 0; i < nl; i++) P.cmap[i] = C.inv[N.cmap[N.perm[i]]];
   rows_of_coarse (P.cmap, C.L.n, P.rptr, P.ridx);
}

}  // namespace mlp

// ================================================================ the plan alone (tests)
extern "C" int nkp_ml_plan_host (int64_t n, const int32_t *rowptr, const int32_t *colind, const double *val, const int32_t *blk_start, int64_t nblk,
                                 const int32_t *col_i, const int32_t *col_j, int coupled_tracer_cnt, int max_levels, int coarsest_rows, int64_t capacity,
                                 int *n_levels, int64_t *rows, int32_t *cmap, int32_t *col_of)
{
   if (n <= 0 || !rowptr || !colind || !val || !blk_start || nblk <= 0 || !n_levels || !rows || !cmap || !col_of) return NKP_EINVAL;
   if (max_levels <= 0) max_levels = 12;
   using namespace mlp;
   std::vector<Nat> nat (1);
   SetupTimes T;
   nkp_tuning tune;
   nkp_default_tuning (&tune);                     // test entry point: defaults + environment
   const PlanKnobs K = plan_knobs (tune);
   init_first_nat (nat[0], n, rowptr, colind, val, blk_start, nblk, col_i, col_j, nullptr, coupled_tracer_cnt, true, K, T);
   extend_nat_levels (nat, 0, (int) nblk, coupled_tracer_cnt, max_levels, coarsest_rows, 0, 0, K, T);
   if (tune.plan_times) printf ("nkp_ml_plan_host: %.2f s low-order twin, %.2f s graphs + aggregation, %.2f s Galerkin products\n", T.low, T.graph, T.galerkin);
   *n_levels = (int) nat.size ();
   int64_t qc = 0, qo = 0;
   for (size_t l = 0; l < nat.size (); l++) {
      rows[l] = nat[l].L.n;
      if (l + 1 < nat.size ()) {
         if (qc + nat[l].L.n > capacity || qo + nat[l + 1].L.n > capacity) return NKP_ENOMEM;
         std::copy (nat[l].cmap.begin (), nat[l].cmap.end (), cmap + qc);
         std::copy (nat[l + 1].col_of.begin (), nat[l + 1].col_of.end (), col_of + qo);
         qc += nat[l].L.n;
         qo += nat[l + 1].L.n;
      }
   }
   return 0;
}
