// What the SpMV kernels (hip_kernels.hip), the BLAS-1 / PCG sweeps (hip_sweeps.hip), the kernels of several
// right-hand sides (hip_mrhs.hip) and the launchers of the AMG cycles (hip_amg*.hip, hip_mrhs_amg.hip) share.
// Included by kernel files only.
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

// lanes per row as the row kernels are instantiated -- 2 .. 32; any other count takes a whole wavefront -- and
// the launchers' dispatch on them: CALL sees the count as the constant L
static inline unsigned row_lanes(unsigned L) { return L == 2 || L == 4 || L == 8 || L == 16 || L == 32 ? L : 64; }

#define LANES_DISPATCH(lanes, CALL)                                            \
  do {                                                                         \
    switch (row_lanes(lanes)) {                                                \
    case 2: { constexpr int L = 2; CALL; } break;                              \
    case 4: { constexpr int L = 4; CALL; } break;                              \
    case 8: { constexpr int L = 8; CALL; } break;                              \
    case 16: { constexpr int L = 16; CALL; } break;                            \
    case 32: { constexpr int L = 32; CALL; } break;                            \
    default: { constexpr int L = 64; CALL; } break;                            \
    }                                                                          \
  } while (0)

#endif
