// What the SpMV kernels (hip_kernels.hip), the BLAS-1 / PCG sweeps (hip_sweeps.hip) and the kernels of
// several right-hand sides (hip_mrhs.hip) share.  Included by those files only.
#ifndef LSB_HIP_KCOMMON_H
#define LSB_HIP_KCOMMON_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "hip_ar.h"
#include "lsb_impl.h"

#include "hip_wg.h"
static_assert(WG == AR_WG, "the folded all-reduce phases assume this workgroup size");

// p_new = D^-1 r + beta p_old: ONE expression for every kernel that forms a direction
// (k_pcg_update_p, k_spmv_subwave_p, k_pcg_col_px), so that their bits agree.
__device__ __forceinline__ double pnew_of(double d, double r, double beta, double p) {
  return __fma_rn(beta, p, d * r);
}

// host helpers of the launchers
static inline unsigned div_up(unsigned a, unsigned b) { return (a + b - 1) / b; }
static inline unsigned round_up(unsigned a, unsigned b) { return div_up(a, b) * b; }
static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

#endif
