// nkp_refactor: new values on the pattern of an existing hierarchy.
//
// Everything the setup decided from the pattern and the coarse cells stays: allocations, colour-major orders, row blocks,
// lane layouts, transfer maps.  What changes is a stream over entries per level:
//   twin      L0 = A + D - diag(rowsum D), D_ij = max(0, -a_ij, -a_ji) between water columns (ml_plan.cpp:
//             build_low_order), one thread per row of A in A's stored order, each value written straight into its
//             colour-major slot of level 0 (tslot, built once);
//   Galerkin  every entry of level l + 1 is the sum of its fine entries of level l, in the order the setup summed them:
//             ascending fine row, then stored position, both in the fine level's NATURAL numbering (gptr / gidx, built
//             once from the colour-major operators and MlLevel::nat_inv);
// then the numeric kernels the setup ran: f32 copies, band factors of the column blocks (repacked into the existing lane
// layout), the coarsest dense inverse.  The summation orders and operations are those of the setup, so the values are its
// bits.  The setup does not store couplings that are exactly zero: a stored one that becomes zero, or a dropped one that
// becomes non-zero, is counted as drift by the value passes before anything a solve reads is written (the caller then
// rebuilds the hierarchy).
#include "refactor.h"

#include "mlsetup.h"
#include "ml_plan.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>

#define RF_T 256

namespace {

template <class T>
bool dalloc (RefactorWork &W, T **p, size_t cnt)
{
   void *q = nullptr;
   const size_t b = (cnt ? cnt : 1) * sizeof (T);
   if (hipMalloc (&q, b) != hipSuccess) {
      (void) hipGetLastError ();          // a tolerated failure must not surface as a stale error in the next solve
      return false;
   }
   *p = (T *) q;
   W.bytes += b;
   return true;
}

template <class T>
bool dupload (RefactorWork &W, T **p, const std::vector<T> &src)
{
   if (!dalloc (W, p, src.size ())) return false;
   return src.empty () || hipMemcpy (*p, src.data (), src.size () * sizeof (T), hipMemcpyHostToDevice) == hipSuccess;
}

template <class T>
bool download (std::vector<T> &dst, const T *src, size_t cnt)
{
   dst.resize (cnt);
   return cnt == 0 || hipMemcpy (dst.data (), src, cnt * sizeof (T), hipMemcpyDeviceToHost) == hipSuccess;
}

inline dim3 rows_grid (int64_t n) { return dim3 ((unsigned) ((n + RF_T - 1) / RF_T)); }

}  // namespace

// ---------------------------------------------------------------- kernels
__global__ __launch_bounds__ (RF_T)
void rf_diag_kernel (int64_t n, const int *__restrict__ rowptr, const int *__restrict__ colind, const double *__restrict__ val, int *__restrict__ cnt)
{
   const int64_t i = (int64_t) blockIdx.x * RF_T + threadIdx.x;
   if (i >= n) return;
   double diag = 0.0;                     // the sum of the stored diagonal entries, as nkp_create judged it
   for (int e = rowptr[i]; e < rowptr[i + 1]; e++)
      if (colind[e] == i) diag += val[e];
   if (!(diag != 0.0)) {
      atomicAdd (cnt + 1, 1);
      atomicMin (cnt + 2, (int) i + 1);
   }
}

__global__ __launch_bounds__ (RF_T)
void rf_row_scale_kernel (int64_t n, const int *__restrict__ rowptr, const double *__restrict__ val, double *__restrict__ rs, double *__restrict__ ri)
{
   const int64_t i = (int64_t) blockIdx.x * RF_T + threadIdx.x;
   if (i >= n) return;
   double mx = 0.0;
   for (int e = rowptr[i]; e < rowptr[i + 1]; e++) mx = fmax (mx, fabs (val[e]));
   rs[i] = mx > 0.0 ? 1.0 / mx : 1.0;
   ri[i] = mx > 0.0 ? mx : 1.0;
}

// level-0 twin values (build_low_order's operations in its order), straight into their colour-major slots
__global__ __launch_bounds__ (RF_T)
void rf_twin_kernel (int64_t n, const int *__restrict__ rowptr, const int *__restrict__ colind, const double *__restrict__ val,
                     const int *__restrict__ tslot, double *__restrict__ out, int *__restrict__ drift)
{
   const int64_t i = (int64_t) blockIdx.x * RF_T + threadIdx.x;
   if (i >= n) return;
   double dsum = 0.0, adiag = 0.0;
   int dslot = -1, bad = 0;
   for (int e = rowptr[i]; e < rowptr[i + 1]; e++) {
      const int j = colind[e];
      double a = val[e];
      const int t = tslot[e];           // slot s >= 0 between columns (or the diagonal), -2 - s inside a column, -1 dropped
      if (j == i) { dslot = t; adiag = a; continue; }
      const bool incol = t <= -2;
      if (!incol) {
         // a_ji by bisection in row j (sorted)
         int lo = rowptr[j], hi = rowptr[j + 1];
         while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (colind[mid] < i) lo = mid + 1;
            else hi = mid;
         }
         const double aji = (lo < rowptr[j + 1] && colind[lo] == i) ? val[lo] : 0.0;
         double d = 0.0;
         if (-a > d) d = -a;
         if (-aji > d) d = -aji;
         a += d;
         dsum += d;
      }
      if (incol) out[-2 - t] = a;                  // always stored
      else if (t >= 0) {
         out[t] = a;
         if (a == 0.0) bad++;                      // the setup would not store it
      } else if (a != 0.0) bad++;                  // ... would store it, but the pattern has no slot
   }
   if (dslot >= 0) out[dslot] = adiag - dsum;
   if (bad) atomicAdd (drift, bad);
}

// Galerkin values of one coarse level: one thread per coarse row, every slot the sum of its fine entries in setup order
__global__ __launch_bounds__ (RF_T)
void rf_galerkin_kernel (int64_t nc, const int *__restrict__ crow, const int *__restrict__ ccol, const int *__restrict__ gptr, const int *__restrict__ gidx,
                         const double *__restrict__ fine, double *__restrict__ out, int *__restrict__ drift)
{
   const int64_t I = (int64_t) blockIdx.x * RF_T + threadIdx.x;
   if (I >= nc) return;
   int bad = 0;
   for (int s = crow[I]; s < crow[I + 1]; s++) {
      double acc = 0.0;
      for (int k = gptr[s]; k < gptr[s + 1]; k++) acc += fine[gidx[k]];
      out[s] = acc;
      if (acc == 0.0 && ccol[s] != I) bad++;
   }
   if (bad) atomicAdd (drift, bad);
}

// coarse pairs the setup dropped as exact zeros: drift if one of them now sums to a non-zero value
__global__ __launch_bounds__ (RF_T)
void rf_phantom_kernel (int nph, const int *__restrict__ pptr, const int *__restrict__ pidx, const double *__restrict__ fine, int *__restrict__ drift)
{
   const int q = blockIdx.x * RF_T + threadIdx.x;
   if (q >= nph) return;
   double acc = 0.0;
   for (int k = pptr[q]; k < pptr[q + 1]; k++) acc += fine[pidx[k]];
   if (acc != 0.0) atomicAdd (drift, 1);
}

// ---------------------------------------------------------------- host side
size_t rf_free_maps (RefactorWork &W)
{
   for (RefactorWork::Lev &L : W.lev)
      for (void *p : { (void *) L.nv, (void *) L.gptr, (void *) L.gidx, (void *) L.pptr, (void *) L.pidx, (void *) L.gcols })
         if (p) (void) hipFree (p);
   if (W.tslot) (void) hipFree (W.tslot);
   if (W.col_gcols) (void) hipFree (W.col_gcols);
   W.lev.clear ();
   W.tslot = nullptr;
   W.col_gcols = nullptr;
   W.col_gcols_done = false;
   W.last_rowptr.clear ();
   W.last_colind.clear ();
   W.maps = false;
   const size_t freed = W.bytes;      // everything but the staging buffers
   W.bytes = 0;
   return freed;
}

void rf_free (RefactorWork &W)
{
   rf_drop_inverse (W);
   rf_free_maps (W);
   if (W.aval) (void) hipFree (W.aval);
   if (W.dcnt) (void) hipFree (W.dcnt);
   W.aval = nullptr;
   W.dcnt = nullptr;
}

int rf_stage (RefactorWork &W, int64_t nnz, int nlev)
{
   // the staging buffers are not counted in W.bytes (they outlive a rebuild of the maps); the caller counts them
   if (!W.aval && hipMalloc ((void **) &W.aval, ((size_t) nnz + 2) * sizeof (double)) != hipSuccess) { (void) hipGetLastError (); W.aval = nullptr; return -2; }
   if (!W.dcnt && hipMalloc ((void **) &W.dcnt, (size_t) (4 + 2 * 64) * sizeof (int)) != hipSuccess) { (void) hipGetLastError (); W.dcnt = nullptr; return -2; }
   return nlev <= 64 ? 0 : -2;
}

void rf_launch_diag_check (const CsrDev &A, const double *val, int *dcnt, hipStream_t st)
{
   (void) hipMemsetAsync (dcnt + 1, 0, sizeof (int), st);
   (void) hipMemsetAsync (dcnt + 2, 0x7f, sizeof (int), st);
   if (A.n) hipLaunchKernelGGL (rf_diag_kernel, rows_grid (A.n), dim3 (RF_T), 0, st, A.n, A.rowptr, A.colind, val, dcnt);
}

void rf_launch_row_scale (const CsrDev &A, const double *val, double *rscale, double *rinv, hipStream_t st)
{
   if (A.n) hipLaunchKernelGGL (rf_row_scale_kernel, rows_grid (A.n), dim3 (RF_T), 0, st, A.n, A.rowptr, val, rscale, rinv);
}

namespace {

// run fn (first, last) on contiguous chunks of [0, n), one host thread each (the setup's thread count)
template <class F>
void par_chunks (int64_t n, int nt, F fn)
{
   if (nt <= 1 || n < 4096) { fn ((int64_t) 0, n); return; }
   std::vector<std::thread> pool;
   for (int t = 0; t < nt; t++) pool.emplace_back ([&, t] () { fn (n * t / nt, n * (t + 1) / nt); });
   for (std::thread &th : pool) th.join ();
}

// slot of column col in row row of a sorted CSR, -1 if absent
inline int find_slot (const std::vector<int> &r, const std::vector<int> &c, int row, int col)
{
   const auto b = c.begin () + r[row], e = c.begin () + r[row + 1];
   const auto q = std::lower_bound (b, e, col);
   return (q < e && *q == col) ? (int) (q - c.begin ()) : -1;
}

}  // namespace

int rf_build_maps (RefactorWork &W, const MlHierarchy &H, const CsrDev &A, hipStream_t st)
{
   const int nlev = (int) H.lev.size ();
   if (nlev < 2 || !H.default_build || !H.perm0 || !H.lev[0].B.blk_start || H.lev[0].n != A.n) return 1;
   for (int l = 1; l < nlev - 1; l++)
      if ((int64_t) H.lev[l].nat_inv.size () != H.lev[l].n) return 1;
   if (hipStreamSynchronize (st) != hipSuccess) return -3;
   rf_free_maps (W);
   const nkp_tuning &T = H.tune ? *H.tune : nkp_builtin_tuning ();
   const int nt = mlp::setup_thread_count (T);
   // host copies of the pattern: A (natural order), every level (colour-major), the transfer maps
   std::vector<int> arp, aci, perm0, blk0;
   std::vector<std::vector<int>> rp (nlev), ci (nlev), cmap (nlev), rptr (nlev), ridx (nlev);
   bool ok = download (arp, A.rowptr, (size_t) A.n + 1) && download (aci, A.colind, (size_t) A.nnz) && download (perm0, H.perm0, (size_t) A.n) &&
             download (blk0, H.lev[0].B.blk_start, (size_t) H.lev[0].B.nblk + 1);
   for (int l = 0; ok && l < nlev; l++) {
      const MlLevel &V = H.lev[l];
      ok = download (rp[l], V.L.rowptr, (size_t) V.n + 1) && download (ci[l], V.L.colind, (size_t) V.L.nnz);
      if (ok && l < nlev - 1)
         ok = V.cmap && V.rptr && V.ridx && download (cmap[l], V.cmap, (size_t) V.n) && download (rptr[l], V.rptr, (size_t) V.nc + 1) &&
              download (ridx[l], V.ridx, (size_t) V.n);
   }
   if (!ok) return -3;
   W.lev.resize (nlev);
   // ---- twin: A entry -> level-0 slot
   {
      const int64_t n = A.n;
      std::vector<int> inv0 ((size_t) n), colcm ((size_t) n), ts ((size_t) A.nnz);
      for (int64_t i = 0; i < n; i++) inv0[perm0[i]] = (int) i;
      for (int c = 0; c + 1 < (int) blk0.size (); c++)
         for (int r = blk0[c]; r < blk0[c + 1]; r++) colcm[r] = c;
      std::atomic<bool> bad { false };
      par_chunks (n, nt, [&] (int64_t i0, int64_t i1) {
         for (int64_t i = i0; i < i1; i++) {
            const int pi = inv0[i];
            for (int e = arp[i]; e < arp[i + 1]; e++) {
               const int j = aci[e], pj = inv0[j];
               const int s = find_slot (rp[0], ci[0], pi, pj);
               const bool incol = colcm[pi] == colcm[pj];
               if ((j == i || incol) && s < 0) bad = true;                   // not the pattern the setup builds
               ts[e] = (j != i && incol) ? -2 - s : s;                        // the sign carries the in-column tag: every int32 slot fits
            }
         }
      });
      if (bad) return 1;
      if (!dupload (W, &W.tslot, ts)) return -2;
   }
   // ---- Galerkin: coarse slot -> its fine entries, in the fine level's natural (row, position) order.  A coarse row's slots
   // get contributions from its own fine rows only, so chunks of coarse rows are independent.
   for (int l = 1; l < nlev; l++) {
      const int f = l - 1;
      const int64_t nf = H.lev[f].n, nc = H.lev[l].n;
      std::vector<int> perm ((size_t) nf);                 // colour-major -> natural
      if (f == 0) perm = perm0;
      else for (int64_t o = 0; o < nf; o++) perm[H.lev[f].nat_inv[o]] = (int) o;
      const std::vector<int> &frp = rp[f], &fci = ci[f], &crp = rp[l], &cci = ci[l], &cm = cmap[f], &rq = rptr[f], &ri = ridx[f];
      const size_t nnzc = cci.size ();
      std::vector<int> key (fci.size ()), gptr (nnzc + 1, 0);
      // pass 1: slot of every fine entry (-1: a pair the setup dropped) and contributions per slot
      par_chunks (nc, nt, [&] (int64_t I0, int64_t I1) {
         for (int64_t I = I0; I < I1; I++)
            for (int q = rq[I]; q < rq[I + 1]; q++) {
               const int i = ri[q];
               for (int e = frp[i]; e < frp[i + 1]; e++) {
                  const int s = find_slot (crp, cci, (int) I, cm[fci[e]]);
                  key[e] = s;
                  if (s >= 0) gptr[(size_t) s + 1]++;
               }
            }
      });
      for (size_t s = 0; s < nnzc; s++) gptr[s + 1] += gptr[s];
      std::vector<int> gidx ((size_t) gptr[nnzc]);
      // pass 2: every coarse row's fine rows in natural order, each row's entries in natural column order
      std::vector<std::vector<std::pair<long long, int>>> ph_parts (nt > 1 ? nt : 1);
      std::atomic<int> part { 0 };
      par_chunks (nc, nt, [&] (int64_t I0, int64_t I1) {
         std::vector<std::pair<long long, int>> ph;
         std::vector<std::pair<int, int>> rows, tmp;
         std::vector<int> cur;
         for (int64_t I = I0; I < I1; I++) {
            rows.clear ();
            for (int q = rq[I]; q < rq[I + 1]; q++) rows.emplace_back (perm[ri[q]], ri[q]);
            std::sort (rows.begin (), rows.end ());
            cur.assign (gptr.begin () + crp[I], gptr.begin () + crp[I + 1]);
            for (const auto &r : rows) {
               const int i = r.second;
               tmp.clear ();
               for (int e = frp[i]; e < frp[i + 1]; e++) tmp.emplace_back (perm[fci[e]], e);
               std::sort (tmp.begin (), tmp.end ());
               for (const auto &t : tmp) {
                  const int e = t.second, s = key[e];
                  if (s >= 0) gidx[(size_t) cur[s - crp[I]]++] = e;
                  else ph.emplace_back ((long long) I * nc + cm[fci[e]], e);
               }
            }
         }
         // chunks are ascending in I; a pair's entries all come from one chunk, in setup order
         std::stable_sort (ph.begin (), ph.end (), [] (const std::pair<long long, int> &a, const std::pair<long long, int> &b) { return a.first < b.first; });
         ph_parts[(size_t) part++].swap (ph);
      });
      std::vector<int> pptr (1, 0), pidx;
      for (const auto &pp : ph_parts)
         for (size_t k = 0; k < pp.size (); k++) {
            if (k == 0 || pp[k].first != pp[k - 1].first) pptr.push_back (pptr.back ());
            pidx.push_back (pp[k].second);
            pptr.back ()++;
         }
      RefactorWork::Lev &L = W.lev[l];
      L.nph = (int) pptr.size () - 1;
      if (!(dupload (W, &L.gptr, gptr) && dupload (W, &L.gidx, gidx))) return -2;
      if (L.nph && !(dupload (W, &L.pptr, pptr) && dupload (W, &L.pidx, pidx))) return -2;
   }
   for (int l = 0; l < nlev; l++) {
      const MlLevel &V = H.lev[l];
      if (!dalloc (W, &W.lev[l].nv, (size_t) V.L.nnz)) return -2;
      if (V.B.fac && V.B.grp_cols && !V.B.grp_cols->empty () && !dupload (W, &W.lev[l].gcols, *V.B.grp_cols)) return -2;
   }
   W.last_rowptr.swap (rp[nlev - 1]);
   W.last_colind.swap (ci[nlev - 1]);
   W.maps = true;
   return 0;
}

void rf_values (RefactorWork &W, const MlHierarchy &H, const CsrDev &A, const double *val, hipStream_t st)
{
   (void) hipMemsetAsync (W.dcnt, 0, sizeof (int), st);
   if (A.n) hipLaunchKernelGGL (rf_twin_kernel, rows_grid (A.n), dim3 (RF_T), 0, st, A.n, A.rowptr, A.colind, val, (const int *) W.tslot, W.lev[0].nv, W.dcnt);
   for (size_t l = 1; l < H.lev.size (); l++) {
      const MlLevel &V = H.lev[l];
      const RefactorWork::Lev &L = W.lev[l];
      if (V.n) hipLaunchKernelGGL (rf_galerkin_kernel, rows_grid (V.n), dim3 (RF_T), 0, st, V.n, V.L.rowptr, V.L.colind, (const int *) L.gptr, (const int *) L.gidx,
                                   (const double *) W.lev[l - 1].nv, L.nv, W.dcnt);
      if (L.nph) hipLaunchKernelGGL (rf_phantom_kernel, rows_grid (L.nph), dim3 (RF_T), 0, st, L.nph, (const int *) L.pptr, (const int *) L.pidx, (const double *) W.lev[l - 1].nv, W.dcnt);
   }
}

#define RF_FAIL(code, ...) do { snprintf (err, errlen, __VA_ARGS__); return (code); } while (0)

int rf_commit (RefactorWork &W, MlHierarchy &H, hipStream_t st, char *err, size_t errlen, int *replaced)
{
   *replaced = 0;
   const int nlev = (int) H.lev.size ();
   (void) hipMemsetAsync (W.dcnt + 4, 0, (size_t) 2 * nlev * sizeof (int), st);
   for (int l = 0; l < nlev; l++) {
      MlLevel &V = H.lev[l];
      const double *nv = W.lev[l].nv;
      if (V.L.val && V.L.nnz) (void) hipMemcpyAsync (V.L.val, nv, (size_t) V.L.nnz * sizeof (double), hipMemcpyDeviceToDevice, st);
      if (V.L.valf && V.L.nnz) mls::to_float (nv, V.L.valf, V.L.nnz, st);
      launch_diag_fill (V.L, st);         // the per-column diagonals, where the level has them, hold the same values
      if (V.B.fac) {
         CsrDev t = V.L;                  // the f64 values the setup factored (the level keeps only the f32 copy in f32 storage mode)
         t.val = const_cast<double *> (nv);
         launch_colblock_factor (t, V.B, W.dcnt + 4 + 2 * l, st);
         if (colblock_repack_lane_layout (V.B, W.lev[l].gcols, st)) RF_FAIL (-3, "nkp_refactor: lane layout of level %d could not be refreshed", l);
      }
   }
   std::vector<int> stat ((size_t) 2 * nlev);
   if (hipMemcpyAsync (stat.data (), W.dcnt + 4, stat.size () * sizeof (int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize (st) != hipSuccess)
      RF_FAIL (-3, "nkp_refactor: factoring the column blocks failed on the device");
   for (int l = 0; l < nlev; l++)
      if (stat[(size_t) 2 * l]) RF_FAIL (-4, "nkp_refactor: zero pivot in a column block of level %d (row %d)", l, stat[(size_t) 2 * l] - 1);
   if (H.coarse_inv && W.inv_new) {
      const MlLevel &V = H.lev[nlev - 1];
      const size_t nn = (size_t) V.n * (size_t) V.n;
      H.inverse_pivoted = W.inv_pivoted;
      if (rf_inverse_same_storage (W, H)) {
         // same storage: into the buffers the cycle (and every clone) already points at
         bool ok = hipMemcpyAsync (H.coarse_inv, W.inv_new, nn * sizeof (double), hipMemcpyDeviceToDevice, st) == hipSuccess;
         if (ok && W.invf_new) ok = hipMemcpyAsync (H.coarse_invf, W.invf_new, (size_t) V.n * W.ldf_new * sizeof (float), hipMemcpyDeviceToDevice, st) == hipSuccess;
         ok = hipStreamSynchronize (st) == hipSuccess && ok;
         rf_drop_inverse (W);
         if (!ok) RF_FAIL (-3, "nkp_refactor: copy of the coarsest inverse failed");
      } else {
         // the blocked elimination and the pivoted routine disagree with the last setup on the storage: new buffers (the
         // caller has refused this while clones are alive)
         (void) hipFree (H.coarse_inv);
         H.device_bytes -= nn * sizeof (double);
         if (H.coarse_invf) { (void) hipFree (H.coarse_invf); H.device_bytes -= (size_t) V.n * H.coarse_ldf * sizeof (float); }
         H.coarse_inv = W.inv_new;
         H.coarse_invf = W.invf_new;
         if (W.invf_new) H.coarse_ldf = W.ldf_new;
         H.device_bytes += W.inv_bytes;
         W.inv_new = nullptr;
         W.invf_new = nullptr;
         *replaced = 1;
      }
   }
   return 0;
}

bool rf_inverse_same_storage (const RefactorWork &W, const MlHierarchy &H)
{
   return (W.invf_new != nullptr) == (H.coarse_invf != nullptr) && (!W.invf_new || W.ldf_new == H.coarse_ldf);
}

void rf_drop_inverse (RefactorWork &W)
{
   if (W.inv_new) (void) hipFree (W.inv_new);
   if (W.invf_new) (void) hipFree (W.invf_new);
   W.inv_new = nullptr;
   W.invf_new = nullptr;
   W.inv_bytes = 0;
}

int rf_prepare_inverse (RefactorWork &W, const MlHierarchy &H, hipStream_t st, char *err, size_t errlen)
{
   rf_drop_inverse (W);
   if (!H.coarse_inv) return 0;
   const int nlev = (int) H.lev.size ();
   const MlLevel &V = H.lev[nlev - 1];
   std::vector<double> hv;
   if (hipStreamSynchronize (st) != hipSuccess || !download (hv, W.lev[nlev - 1].nv, (size_t) V.L.nnz)) RF_FAIL (-3, "nkp_refactor: download of the coarsest operator failed");
   const int irc = ml_coarse_inverse (H, (int) V.n, W.last_rowptr.data (), W.last_colind.data (), hv.data (), &W.inv_new, &W.invf_new, &W.ldf_new, &W.inv_bytes, st);
   if (irc == -4) RF_FAIL (-4, "nkp_refactor: the coarsest operator of the new values is singular (or the device is out of memory); the solver is unchanged");
   if (irc < 0) { (void) hipGetLastError (); RF_FAIL (-2, "nkp_refactor: device allocation failed (dense inverse of %lld rows)", (long long) V.n); }
   W.inv_pivoted = irc == 1;
   return 0;
}

int rf_column_factor (RefactorWork &W, const CsrDev &A, ColBlocksDev &B, hipStream_t st, char *err, size_t errlen)
{
   if (!W.col_gcols_done) {
      if (B.grp_cols && !B.grp_cols->empty () && !dupload (W, &W.col_gcols, *B.grp_cols)) RF_FAIL (-2, "nkp_refactor: device allocation failed");
      W.col_gcols_done = true;
   }
   (void) hipMemsetAsync (W.dcnt + 4, 0, 2 * sizeof (int), st);
   launch_colblock_factor (A, B, W.dcnt + 4, st);
   if (colblock_repack_lane_layout (B, W.col_gcols, st)) RF_FAIL (-3, "nkp_refactor: lane layout of the column blocks could not be refreshed");
   int stat[2] = { 0, 0 };
   if (hipMemcpyAsync (stat, W.dcnt + 4, sizeof stat, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize (st) != hipSuccess)
      RF_FAIL (-3, "nkp_refactor: factoring the column blocks failed on the device");
   if (stat[0]) RF_FAIL (-4, "nkp_refactor: zero pivot at row %d while factoring its water-column block", stat[0] - 1);
   return 0;
}
#undef RF_FAIL
