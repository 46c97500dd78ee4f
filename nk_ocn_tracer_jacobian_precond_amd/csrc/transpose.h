// The device transpose of transpose.hip, shared with transpose_dist.hip.  Private to the library.
#pragma once
#include "nkp_dev.h"
#include "mlsetup.h"

// A^T of the device CSR A of A.n rows and ncols columns: rowptrT[ncols + 1], colindT / valT / src[nnz] (valT[p] = val[src[p]]),
// every row sorted by column.  Synchronises st.  0, a hipError_t, or 1000 for inconsistent column counts
NKP_PRIVATE int transpose_device (const CsrDev &A, int64_t ncols, mls::DBuf<int> &rowptrT, mls::DBuf<int> &colindT, mls::DBuf<double> &valT, mls::DBuf<int> &src, hipStream_t st);
