// Host planner of the multilevel preconditioner (ml_plan.cpp): plain C++, no HIP.  What multilevel.hip (and the thread count
// refactor.hip) needs of it; private to the library.
#pragma once
#include "../../include/nkp.h"
#include "tuning.h"

#include <stdint.h>

#include <algorithm>
#include <thread>
#include <utility>
#include <vector>

namespace mlp {

// allocator whose resize () leaves the new elements uninitialised: the setup's big arrays are written once by row-parallel
// loops right after they are sized, and a zero-fill by ONE thread (page faults included) was most of the "twin" time
template <class T>
struct RawAlloc {
   using value_type = T;
   RawAlloc () = default;
   template <class U> RawAlloc (const RawAlloc<U> &) {}
   T *allocate (size_t k) { return static_cast<T *> (::operator new (k * sizeof (T))); }
   void deallocate (T *q, size_t) { ::operator delete (q); }
   template <class U> void construct (U *q) noexcept { ::new ((void *) q) U; }                       // default-init: no store for int / double
   template <class U, class... A> void construct (U *q, A &&... a) { ::new ((void *) q) U (std::forward<A> (a)...); }
   template <class U> bool operator== (const RawAlloc<U> &) const { return true; }
   template <class U> bool operator!= (const RawAlloc<U> &) const { return false; }
};
using RawInts = std::vector<int, RawAlloc<int>>;
using RawDoubles = std::vector<double, RawAlloc<double>>;

struct HostCsr {
   int64_t n = 0;
   std::vector<int> rowptr;
   RawInts colind;
   RawDoubles val;
};

// host threads of the setup loops (1 degree, 256-core host: Galerkin products 0.25 / 0.14 / 0.11 s with 16 / 32 / 64 threads; 32
// leaves room for one process per GPU on an 8-GPU node)
inline int setup_thread_count (const nkp_tuning &t)
{
   return t.setup_threads > 0 ? t.setup_threads : (int) std::min (32u, std::max (1u, std::thread::hardware_concurrency ()));
}

// run fn (chunk, first_row, last_row) on contiguous row chunks, one of `threads` host threads each
template <class F>
void for_row_chunks (int64_t n, int threads, F fn)
{
   const int nt = n < 200000 ? 1 : threads;
   std::vector<std::thread> pool;
   for (int c = 0; c < nt; c++) {
      const int64_t r0 = n * c / nt, r1 = n * (c + 1) / nt;
      if (nt == 1) fn (c, r0, r1);
      else pool.emplace_back ([=] () { fn (c, r0, r1); });
   }
   for (std::thread &th : pool) th.join ();
}

// ---------------------------------------------------------------- natural-order data of every level (host)
struct Nat {
   HostCsr L;
   std::vector<int> blk_start, col_of, colour, agg;   // per column: colour, aggregate id
   std::vector<int> cmap;                            // fine row -> coarse row (natural orders)
   std::vector<int> perm, inv;                       // perm[new] = old ; inv[old] = new  (colour-major)
   std::vector<int> pblk;                            // row offsets of the columns in colour-major order
   std::vector<int> gi, gj, gt;                      // optional grid position / tracer of every column
   std::vector<int> ktop;                            // depth of the first row of every column (0 except for stub columns)
   int nagg = 0;
   int ncol0 = 0;                                    // columns of colour 0
};

struct SetupTimes { double low = 0.0, graph = 0.0, galerkin = 0.0; };

// knobs of the hierarchy construction (nkp_tuning; defaults are the measured best), the host threads of
// its row-parallel loops and the timing print of the aggregation
struct PlanKnobs {
   int split = 1, pocket = 4, big_from = -3, huge_from = -1;
   double theta = 0.0, tau = 0.01;
   int threads = 1;
   bool times = false;
};
NKP_PRIVATE PlanKnobs plan_knobs (const nkp_tuning &t);

// level-0 column arrays (and, with_twin, the low-order twin of A on the host)
NKP_PRIVATE void init_first_nat (Nat &N, int64_t n, const int *rowptr, const int *colind, const double *val, const int *blk_start_in, int64_t nblk,
                                 const int *col_i, const int *col_j, const int *col_t, int tracer_cnt, bool with_twin, const PlanKnobs &K, SetupTimes &T);
// 2 x 2 blocks of columns in (i, j) (4 x 4 with sh = 2), never across tracers; group ids in order of first member.
// Returns the number of groups; agg[c] = group of column c, cgi / cgj / cgt = position and tracer of every group.
NKP_PRIVATE int geo_groups (const Nat &N, int sh, std::vector<int> &agg, std::vector<int> &cgi, std::vector<int> &cgj, std::vector<int> &cgt);
// the sh of geo_groups for a level
NKP_PRIVATE int group_shift (const PlanKnobs &K, int level, int ncol_level0, int tracer_cnt);
// the colour-major column order of N.colour: N.pblk, N.ncol0 and newstart[c] = first row of column c in that order
NKP_PRIVATE void colour_major_columns (Nat &N, std::vector<int> &newstart);
// colouring, aggregation and Galerkin product of every level from nat.back () on (which holds its operator).
// level0 = index of nat[0] in the whole hierarchy (levels above it were built on the device).
NKP_PRIVATE void extend_nat_levels (std::vector<Nat> &nat, int level0, int ncol_level0, int tracer_cnt, int max_levels, int coarsest_rows, int verbose,
                                    int rank, const PlanKnobs &K, SetupTimes &T);

// a level in colour-major order, as the device holds it: the operator (row new = row perm[new] of N.L, columns relabelled
// through inv and sorted) and, towards a coarser level C, the transfer maps fine row -> coarse row -> its fine rows
struct ColourMajorLevel {
   std::vector<int> prow;
   RawInts pcol;
   RawDoubles pval;
   std::vector<int> cmap, rptr, ridx;
};
NKP_PRIVATE void colour_major_operator (const Nat &N, int threads, ColourMajorLevel &P);
NKP_PRIVATE void colour_major_transfers (const Nat &N, const Nat &C, ColourMajorLevel &P);

// dense inverse by Gauss-Jordan with partial pivoting (coarsest level only); returns false if singular
NKP_PRIVATE bool dense_inverse (int n, std::vector<double> &a /* row-major n*n, overwritten by its inverse */);

}  // namespace mlp
