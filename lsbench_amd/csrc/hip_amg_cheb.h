// The Chebyshev smoother's step on one row, shared by the single-column kernels (hip_amg.hip) and the kernels on
// blocks of columns (hip_amg_cheb.hip): ONE expression, so that a column of a block has the single cycle's bits.
#ifndef LSB_HIP_AMG_CHEB_H
#define LSB_HIP_AMG_CHEB_H
#include <hip/hip_runtime.h>

// the new direction of row i in step k, given s = (A x)_i, dinv = 1 / a_ii and the old direction d:
//   fma(c2 dinv, b - s, c1 d);  c1 == 0 (step 0):  (c2 dinv) (b - s) -- d is uninitialised there, the caller
// does not load it (it passes anything finite) and 0 * NaN cannot arise
__device__ __forceinline__ double amg_cheb_dir(double c1, double c2, double dinv, double b, double s, double d) {
  const double m = c2 * dinv, t = b - s;
  return c1 == 0.0 ? m * t : fma(m, t, c1 * d);
}

#endif
