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

// How a streamed 16-byte store leaves the XCD's L2: ST_KEEP (a plain store) and ST_NT (nontemporal) write the line
// into the L2 and leave it there, dirty, for the write-back at the end of the launch; ST_SC1 / ST_SC1_NT write it
// through (the store's sc1 bit), so the launch ends with nothing of it left to flush.  The last two are the cache-policy
// bits of a buffer store's aux operand (sc1 = 16, nt = 2 on gfx940 and later).
enum { ST_KEEP = 0, ST_NT = 1, ST_SC1 = 16, ST_SC1_NT = 18 };
// One slice's worth of a vector: 64 lanes x 16 bytes at the wave-uniform address `slice`; lane l stores v at
// slice + 2 l.  The write-through forms go through a buffer resource that covers just this slice -- rebased per
// store out of scalar registers, so a vector of 4 GB and more needs no other path, and the lane's offset is the
// one VGPR 16 l.  A builtin, not inline assembly: the compiler counts the store in vmcnt in program order with
// the loads around it, which the column pipelines rely on.
template <int POL, typename V2> __device__ __forceinline__ void slice_store16(double *slice, unsigned lane, V2 v) {
  static_assert(sizeof(V2) == 16, "a pair of doubles");
  if constexpr (POL == ST_KEEP)
    *(V2 *)(slice + 2 * lane) = v;
  else if constexpr (POL == ST_NT)
    __builtin_nontemporal_store(v, (V2 *)(slice + 2 * lane));
  else {
    typedef unsigned st_u4 __attribute__((ext_vector_type(4)));
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(st_u4, v),
                                           __builtin_amdgcn_make_buffer_rsrc(slice, 0, 64 * 16, 0x00020000),
                                           16u * lane, 0, POL);
  }
}

// wg_sum_partials (hip_wg.h) with its loads in flight together.  That loop asks for one record, waits, adds, and
// asks for the next: five dependent round trips for the 1280 records a resident grid of five workgroups per CU
// leaves, at the head of a launch that can do nothing else until it has the sums.  Here a thread asks for U records
// at once and adds them -- and whatever lies beyond U * WG records, batch by batch -- in wg_sum_partials' order:
// record threadIdx.x first, then + WG, ...; the same terms in the same order, so the same bits.
template <int W, int U>
__device__ __forceinline__ void wg_sum_parts(const double *__restrict__ parts, unsigned nparts, double (&v)[W],
                                             double *sred) {
#pragma unroll
  for (int k = 0; k < W; k++)
    v[k] = 0.0;
  for (unsigned base = 0; base < nparts; base += U * WG) {
    double t[U][W];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const unsigned i = base + u * WG + threadIdx.x, ic = i < nparts ? i : 0u; // (every lane loads: no join)
#pragma unroll
      for (int k = 0; k < W; k++)
        t[u][k] = parts[(size_t)ic * W + k];
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const bool have = base + u * WG + threadIdx.x < nparts;
#pragma unroll
      for (int k = 0; k < W; k++)
        v[k] = have ? v[k] + t[u][k] : v[k];
    }
  }
  wg_sum<W>(v, sred);
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
