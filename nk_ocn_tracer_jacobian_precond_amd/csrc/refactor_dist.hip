// nkp_refactor_dist: the values of a distributed rank's hierarchy source from its own new values and the overlap values its
// neighbours ship.  Two gathers on the device around the caller's alltoallv:
//   pack      sendbuf[k] = aval[ship[k]]                                   (own entries of the rows other ranks overlap)
//   assemble  sval[k]    = aval[origin[k]] or recvbuf[-1 - origin[k]]      (the source in its CSR order, flush_row's sorts included)
// The maps are nkp_create_dist's plan (DistRefactorPlan), uploaded at the first call; the value passes of refactor.hip then run
// on the source exactly as they run on a single GPU's matrix.
#include "refactor.h"

#define RFD_T 256

namespace {

template <class T>
bool qalloc (DistRefactorPlan &Q, T **p, size_t cnt)
{
   void *q = nullptr;
   const size_t b = (cnt ? cnt : 1) * sizeof (T);
   if (hipMalloc (&q, b) != hipSuccess) {
      (void) hipGetLastError ();
      return false;
   }
   *p = (T *) q;
   Q.bytes += b;
   return true;
}

template <class T>
bool qupload (DistRefactorPlan &Q, T **p, const std::vector<T> &src, size_t cnt)
{
   if (!qalloc (Q, p, cnt)) return false;
   return cnt == 0 || hipMemcpy (*p, src.data (), cnt * sizeof (T), hipMemcpyHostToDevice) == hipSuccess;
}

inline dim3 grid_of (int64_t n) { return dim3 ((unsigned) ((n + RFD_T - 1) / RFD_T)); }

}  // namespace

__global__ __launch_bounds__ (RFD_T)
void rf_dist_pack_kernel (int64_t n, const int *__restrict__ ship, const double *__restrict__ aval, double *__restrict__ out)
{
   const int64_t k = (int64_t) blockIdx.x * RFD_T + threadIdx.x;
   if (k < n) out[k] = aval[ship[k]];
}

__global__ __launch_bounds__ (RFD_T)
void rf_dist_assemble_kernel (int64_t n, const int *__restrict__ origin, const double *__restrict__ aval, const double *__restrict__ recv,
                              double *__restrict__ out)
{
   const int64_t k = (int64_t) blockIdx.x * RFD_T + threadIdx.x;
   if (k >= n) return;
   const int o = origin[k];
   out[k] = o >= 0 ? aval[o] : recv[-1 - o];
}

int rf_dist_upload (DistRefactorPlan &Q, hipStream_t st)
{
   if (Q.uploaded) return 0;
   if (hipStreamSynchronize (st) != hipSuccess) return -3;
   const size_t nship = Q.ship.size ();
   bool ok = qupload (Q, &Q.src.rowptr, Q.src_rowptr, (size_t) Q.n_src + 1) && qupload (Q, &Q.src.colind, Q.src_colind, (size_t) Q.nnz_src) &&
             qupload (Q, &Q.d_origin, Q.origin, (size_t) Q.nnz_src) && qalloc (Q, &Q.sval, (size_t) Q.nnz_src);
   if (ok && Q.exchange)
      ok = qupload (Q, &Q.d_ship, Q.ship, nship) && qalloc (Q, &Q.sendbuf, nship) && qalloc (Q, &Q.recvbuf, (size_t) Q.n_recv);
   if (!ok) {
      rf_dist_free (Q);
      return -2;
   }
   Q.src.n = Q.n_src;
   Q.src.nnz = Q.nnz_src;
   // the device copies are what the value passes read from now on; a rebuild reads the pattern back
   std::vector<int32_t> ().swap (Q.src_rowptr);
   std::vector<int32_t> ().swap (Q.src_colind);
   std::vector<int32_t> ().swap (Q.origin);
   std::vector<int32_t> ().swap (Q.ship);
   Q.uploaded = true;
   return 0;
}

void rf_dist_free (DistRefactorPlan &Q)
{
   for (void *p : { (void *) Q.src.rowptr, (void *) Q.src.colind, (void *) Q.sval, (void *) Q.sendbuf, (void *) Q.recvbuf, (void *) Q.d_origin, (void *) Q.d_ship })
      if (p) (void) hipFree (p);
   Q.src = CsrDev ();
   Q.sval = Q.sendbuf = Q.recvbuf = nullptr;
   Q.d_origin = Q.d_ship = nullptr;
   Q.bytes = 0;
   Q.uploaded = false;
}

void rf_dist_launch_pack (const DistRefactorPlan &Q, const double *aval, hipStream_t st)
{
   int64_t n = 0;
   for (int c : Q.ship_counts) n += c;
   if (n) hipLaunchKernelGGL (rf_dist_pack_kernel, grid_of (n), dim3 (RFD_T), 0, st, n, (const int *) Q.d_ship, aval, Q.sendbuf);
}

void rf_dist_launch_assemble (const DistRefactorPlan &Q, const double *aval, hipStream_t st)
{
   if (Q.nnz_src) hipLaunchKernelGGL (rf_dist_assemble_kernel, grid_of (Q.nnz_src), dim3 (RFD_T), 0, st, Q.nnz_src, (const int *) Q.d_origin, aval,
                                      (const double *) Q.recvbuf, Q.sval);
}
